// composite.hip.h — the folder driver's frame at the SOURCE resolution, fused on the GPU (rib_composite, include/rib.h).
//
// The generator predicts a person at the model size; the background frame exists at the source size.  composite.py states
// the full-resolution frame in integers (composite_host):
//
//   P  = quantise_u8(pred)              uint8 [H, W, 3]      the PNG quantiser (pixel_ops.hip.h)
//   M  = quantise_mask_u8(mask)         uint8 [H, W]         uint8(clip(m, 0, 1) * 255), in double
//   Pu, Mu = the 8-bit cubic resize of P and M to H0 x W0    (resize.py: 11-bit taps, (v + 2^21) >> 22, saturated)
//   out = (Pu * Mu + bg * (255 - Mu) + 127) / 255            int32, per channel
//
// and this kernel writes the same bytes in one launch.  The per-axis tap tables are resize._cubic_taps' (made on the host and
// uploaded, as for rib_resize_cubic): what is left is integer arithmetic, exact in any summation order.
//
//   k_composite   grid (tiles, N).  A workgroup of 4 waves owns CMP_TW x CMP_TH = 64 x 16 output pixels of one frame; a lane
//                 owns one pixel column and 4 rows.
//                 1. the tile's input patch - the rows and columns its taps reach, found from the tables of the tile's first
//                    and last column / row - is read once from pred's three planes and mask's plane, quantised, and kept in
//                    LDS as one word per input pixel (r, g, b, m in its four bytes): 21 x 11 pixels at 64^2 -> 240 x 136,
//                    67 x 19 at equal sizes;
//                 2. horizontal pass: a lane holds its column's four taps in registers and forms, for every patch row, the
//                    four channels' sums in int32 (LDS, one int4 per patch row and column);
//                 3. vertical pass from those, the fixed-point cast, and the blend with the pixel's own background bytes;
//                 4. background rows arrive and output rows leave as whole dwords: a row segment (192 bytes) is staged in
//                    LDS at its own phase inside a dword, so that an aligned LDS word is an aligned word of global memory;
//                    the partial words at a segment's two ends go as bytes (they belong to the neighbouring tile or row).
//                    A pixel reads no background byte but its own, so out may be bg.
//                 LDS is dynamic: the host sizes the patch and the horizontal sums for the size pair (composite_patch_bound:
//                 20.5 KB at 512^2 -> 1920 x 1080, 7 workgroups per CU; the launch is bound by the latency of its dependent
//                 loads, so resident workgroups are what it needs).  A size pair whose bound exceeds CMP_PW x CMP_PH (a
//                 reduction by more than about 1.06 in x or 1.27 in y) gets no patch at all and every tile takes the plain
//                 path: 16 taps per pixel gathered from global memory and quantised there.  That path is there to be correct
//                 for every size pair, not to be fast.  A workgroup checks its own patch against the bound it was launched
//                 with (tables of a C caller need not be resize._cubic_taps') and takes the plain path if it does not fit;
//                 either path evaluates the same integers.
//
// One launch, no workspace, no atomics: a frame's bytes do not depend on N.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pixel_ops.hip.h"
#include "resize.hip.h"

namespace rib {

#define CMP_TW 64                    // output tile: 64 pixel columns (one per lane of a wave) ...
#define CMP_TH 16                    // ... by 16 rows, 4 per wave
#define CMP_PW 72                    // largest input patch kept in LDS: columns ...
#define CMP_PH 24                    // ... and rows
#define CMP_ROW_WORDS 52             // a staged row segment: 64 * 3 bytes at a phase of 0..3, in whole words (50), padded

struct CompositeParams {
  const float* pred;                 // [N, 3, H, W]
  const float* mask;                 // [N, 1, H, W]
  const uint8_t* bg;                 // [N, H0, W0, 3]
  const int4 *ix, *cx, *iy, *cy;     // [W0], [W0], [H0], [H0]: resize._cubic_taps(W0, W), (H0, H)
  uint8_t* out;                      // [N, H0, W0, 3]; may be bg
  int H, W, H0, W0, tilesX;
  int pwMax, phMax;                  // the patch the launch's LDS was sized for (0, 0: none, every tile takes the plain path)
};

// An upper bound of the input pixels that `tile` consecutive outputs of one axis reach, dst <- src: the taps of output d are
// floor(f(d)) - 1 .. floor(f(d)) + 2 with f(d) = (d + 0.5) * src / dst - 0.5 rounded to float32 (resize._cubic_taps), so the
// first and the last output of a tile are at most floor((tile - 1) * src / dst) + 1 integer positions apart (the 0.01 covers the
// float32 rounding of f for inputs up to 2^15 pixels a side), plus the four taps; clamping to the frame only shrinks it.  Nothing
// rests on the bound but speed: a workgroup whose patch outgrows it takes the plain path (k_composite checks its own patch).
inline int composite_patch_bound(int tile, int dst, int src) {
  const double span = (double)(tile - 1) * (double)src / (double)dst + 0.01;
  return span > 1e6 ? 1 << 20 : (int)span + 5;
}

// dynamic LDS of k_composite for a patch of pw x ph: the horizontal sums, the row taps, the two staged row segments, the patch
inline size_t composite_lds_bytes(int pw, int ph) {
  return (size_t)ph * CMP_TW * 16 + 2 * CMP_TH * 16 + 2 * (size_t)CMP_TH * CMP_ROW_WORDS * 4 + (size_t)pw * ph * 4;
}

__device__ __forceinline__ int cmp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int cmp_min4(int4 v) { return min(min(v.x, v.y), min(v.z, v.w)); }
__device__ __forceinline__ int cmp_max4(int4 v) { return max(max(v.x, v.y), max(v.z, v.w)); }
__device__ __forceinline__ int cmp_pick(int4 v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }   // (no indexed registers)

// one input pixel, quantised: r | g << 8 | b << 16 | m << 24
__device__ __forceinline__ uint32_t cmp_fetch(const float* pred, const float* mask, size_t plane, size_t at) {
  return (uint32_t)quantise_u8(pred[at]) | ((uint32_t)quantise_u8(pred[plane + at]) << 8) |
         ((uint32_t)quantise_u8(pred[2 * plane + at]) << 16) | ((uint32_t)quantise_mask_u8(mask[at]) << 24);
}

// Products go through the 24-bit multiplier (full rate; the 32-bit one is quarter rate): a coefficient is a short, a pixel a byte,
// and a horizontal sum is at most 255 * (1.375 * 2048) < 2^20 in magnitude, so every operand is a 24-bit signed integer and
// the product is the exact one.
__device__ __forceinline__ void cmp_mac(int acc[4], int w, uint32_t px) {
  acc[0] += __mul24(w, (int)(px & 255u));
  acc[1] += __mul24(w, (int)((px >> 8) & 255u));
  acc[2] += __mul24(w, (int)((px >> 16) & 255u));
  acc[3] += __mul24(w, (int)(px >> 24));
}

__device__ __forceinline__ int cmp_cast(int v) {       // FixedPtCast<int, uchar, 22>: arithmetic shift, saturated
  return cmp_clamp((v + (1 << (2 * RSZ_COEF_BITS - 1))) >> (2 * RSZ_COEF_BITS), 0, 255);
}

__global__ __launch_bounds__(256) void k_composite(CompositeParams p) {
  extern __shared__ int4 cmp_lds[];                            // composite_lds_bytes(p.pwMax, p.phMax), in this order:
  int4 (*s_h)[CMP_TW] = reinterpret_cast<int4 (*)[CMP_TW]>(cmp_lds);
  int4* s_iy = cmp_lds + (size_t)p.phMax * CMP_TW;
  int4* s_cy = s_iy + CMP_TH;
  uint32_t (*s_bg)[CMP_ROW_WORDS] = reinterpret_cast<uint32_t (*)[CMP_ROW_WORDS]>(s_cy + CMP_TH);
  uint32_t (*s_out)[CMP_ROW_WORDS] = s_bg + CMP_TH;
  uint32_t* s_patch = reinterpret_cast<uint32_t*>(s_out + CMP_TH);

  const int H = p.H, W = p.W, H0 = p.H0, W0 = p.W0;
  const int tx = blockIdx.x % p.tilesX, ty = blockIdx.x / p.tilesX;
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = tx * CMP_TW, y0 = ty * CMP_TH;
  const int seg = min(CMP_TW, W0 - x0) * 3;                   // bytes of this tile's row segment
  const size_t pitch = (size_t)W0 * 3;

  // the background words of this wave's four rows: asked for first, used last.  A word that lies wholly inside the segment is
  // one load; the words across its ends are put together from the segment's own bytes.
  uint32_t bgw[CMP_TH / 4];
  int pb[CMP_TH / 4];                                         // the phase of each row segment inside a dword
#pragma unroll
  for (int r = 0; r < CMP_TH / 4; ++r) {
    const int y = y0 + wave * (CMP_TH / 4) + r;
    bgw[r] = 0; pb[r] = 0;
    if (y >= H0) continue;
    const uint8_t* bp = p.bg + ((size_t)n * H0 + y) * pitch + (size_t)x0 * 3;
    pb[r] = (int)(reinterpret_cast<uintptr_t>(bp) & 3);
    const int lo = lane * 4 - pb[r];                          // where the lane's word starts, in bytes of the segment
    if (lo >= 0 && lo + 4 <= seg) {
      bgw[r] = *reinterpret_cast<const uint32_t*>(bp + lo);
    } else if (lo < seg) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lo + q >= 0 && lo + q < seg) bgw[r] |= (uint32_t)bp[lo + q] << (8 * q);
    }
  }

  if (threadIdx.x < CMP_TH) {
    const int y = min(y0 + (int)threadIdx.x, H0 - 1);         // (rows past the frame are never read back)
    s_iy[threadIdx.x] = p.iy[y];
    s_cy[threadIdx.x] = p.cy[y];
  }
  // the input patch, from the tables of the tile's first and last column and row (the tables are monotone; a tap that a bad
  // table of a C caller points elsewhere is clamped into the patch below, and into the frame on the plain path)
  const int xl = min(x0 + CMP_TW - 1, W0 - 1), yl = min(y0 + CMP_TH - 1, H0 - 1);
  const int px_lo = cmp_clamp(cmp_min4(p.ix[x0]), 0, W - 1), px_hi = cmp_clamp(cmp_max4(p.ix[xl]), 0, W - 1);
  const int py_lo = cmp_clamp(cmp_min4(p.iy[y0]), 0, H - 1), py_hi = cmp_clamp(cmp_max4(p.iy[yl]), 0, H - 1);
  const int pw = px_hi - px_lo + 1, ph = py_hi - py_lo + 1;
  const bool staged = pw >= 1 && pw <= p.pwMax && ph >= 1 && ph <= p.phMax;      // the same for the whole workgroup

  const int x = min(x0 + lane, W0 - 1);                       // (columns past the frame compute the last one and store nothing)
  const int4 tix = p.ix[x], tcx = p.cx[x];
  const int gx[4] = {cmp_clamp(tix.x, 0, W - 1), cmp_clamp(tix.y, 0, W - 1), cmp_clamp(tix.z, 0, W - 1), cmp_clamp(tix.w, 0, W - 1)};
  const int wx[4] = {tcx.x, tcx.y, tcx.z, tcx.w};
  const size_t plane = (size_t)H * W;
  const float* pred = p.pred + (size_t)n * 3 * plane;
  const float* mask = p.mask + (size_t)n * plane;

  // exact in int32 as in OpenCV: |v| <= 255 * (1.375 * 2048)^2 < 2^31, which also covers v + 2^21 in cmp_cast
  int v[CMP_TH / 4][4];
#pragma unroll
  for (int r = 0; r < CMP_TH / 4; ++r) v[r][0] = v[r][1] = v[r][2] = v[r][3] = 0;

  if (staged) {
    for (int i = threadIdx.x; i < pw * ph; i += 256) {
      const int py = i / pw, px = i - py * pw;
      s_patch[i] = cmp_fetch(pred, mask, plane, (size_t)(py_lo + py) * W + (px_lo + px));
    }
    __syncthreads();
    const int lx[4] = {cmp_clamp(gx[0] - px_lo, 0, pw - 1), cmp_clamp(gx[1] - px_lo, 0, pw - 1),
                       cmp_clamp(gx[2] - px_lo, 0, pw - 1), cmp_clamp(gx[3] - px_lo, 0, pw - 1)};
    for (int py = wave; py < ph; py += 4) {
      const uint32_t* row = s_patch + py * pw;
      int a[4] = {0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 4; ++i) cmp_mac(a, wx[i], row[lx[i]]);
      s_h[py][lane] = make_int4(a[0], a[1], a[2], a[3]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CMP_TH / 4; ++r) {
      const int ry = wave * (CMP_TH / 4) + r;
      const int4 tiy = s_iy[ry], tcy = s_cy[ry];
      const int ly[4] = {cmp_clamp(cmp_clamp(tiy.x, 0, H - 1) - py_lo, 0, ph - 1), cmp_clamp(cmp_clamp(tiy.y, 0, H - 1) - py_lo, 0, ph - 1),
                         cmp_clamp(cmp_clamp(tiy.z, 0, H - 1) - py_lo, 0, ph - 1), cmp_clamp(cmp_clamp(tiy.w, 0, H - 1) - py_lo, 0, ph - 1)};
      const int wy[4] = {tcy.x, tcy.y, tcy.z, tcy.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int4 hs = s_h[ly[j]][lane];
        v[r][0] += __mul24(wy[j], hs.x); v[r][1] += __mul24(wy[j], hs.y); v[r][2] += __mul24(wy[j], hs.z); v[r][3] += __mul24(wy[j], hs.w);
      }
    }
  } else {
    __syncthreads();                                          // s_iy, s_cy
#pragma unroll
    for (int r = 0; r < CMP_TH / 4; ++r) {                    // (v[r] stays in registers; the taps below are not unrolled)
      const int ry = wave * (CMP_TH / 4) + r;
      if (y0 + ry >= H0) break;
      const int4 tiy = s_iy[ry], tcy = s_cy[ry];
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {                           // rolled: this path is short on registers by design, not fast
        const size_t row = (size_t)cmp_clamp(cmp_pick(tiy, j), 0, H - 1) * W;
        int a[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int i = 0; i < 4; ++i)
          cmp_mac(a, cmp_pick(tcx, i), cmp_fetch(pred, mask, plane, row + cmp_clamp(cmp_pick(tix, i), 0, W - 1)));
        const int wy = cmp_pick(tcy, j);
        v[r][0] += __mul24(wy, a[0]); v[r][1] += __mul24(wy, a[1]); v[r][2] += __mul24(wy, a[2]); v[r][3] += __mul24(wy, a[3]);
      }
    }
  }

  // the background rows into LDS at their phase, the blend, the output rows out of LDS at theirs
#pragma unroll
  for (int r = 0; r < CMP_TH / 4; ++r)
    if (lane < CMP_ROW_WORDS) s_bg[wave * (CMP_TH / 4) + r][lane] = bgw[r];
  __syncthreads();
  int po[CMP_TH / 4];
#pragma unroll
  for (int r = 0; r < CMP_TH / 4; ++r) {
    const int ry = wave * (CMP_TH / 4) + r;
    const int y = y0 + ry;
    po[r] = 0;
    if (y >= H0) continue;
    po[r] = (int)(reinterpret_cast<uintptr_t>(p.out + ((size_t)n * H0 + y) * pitch + (size_t)x0 * 3) & 3);
    if (x0 + lane >= W0) continue;
    const uint8_t* bgrow = reinterpret_cast<const uint8_t*>(s_bg[ry]) + pb[r] + lane * 3;
    uint8_t* orow = reinterpret_cast<uint8_t*>(s_out[ry]) + po[r] + lane * 3;
    const int m = cmp_cast(v[r][3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) orow[c] = (uint8_t)((cmp_cast(v[r][c]) * m + (int)bgrow[c] * (255 - m) + 127) / 255);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < CMP_TH / 4; ++r) {
    const int ry = wave * (CMP_TH / 4) + r;
    const int y = y0 + ry;
    if (y >= H0) continue;
    uint8_t* op = p.out + ((size_t)n * H0 + y) * pitch + (size_t)x0 * 3;
    const int lo = lane * 4 - po[r];
    if (lo >= seg) continue;
    if (lo >= 0 && lo + 4 <= seg) {
      *reinterpret_cast<uint32_t*>(op + lo) = s_out[ry][lane];
    } else {
      const uint8_t* b = reinterpret_cast<const uint8_t*>(&s_out[ry][lane]);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lo + q >= 0 && lo + q < seg) op[lo + q] = b[q];
    }
  }
}

}  // namespace rib
