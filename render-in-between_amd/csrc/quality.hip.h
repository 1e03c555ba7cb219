// quality.hip.h — masked PSNR / SSIM of rendered frames against ground truth (rib_quality, include/rib.h).
//
// The metric is the reference's Evaluator.compute_metrics (PGNR/models/evaluator.py:149-163) with piq's defaults,
// psnr(data_range=1, reduction='mean') and ssim(data_range=1), restated from piq (unpinned: piq is not a dependency):
//
//   x = clamp(pred*0.5+0.5, 0, 1) * mask, y = the same of target (mask [B,H,W], broadcast over the channels, or none)
//   PSNR  = -10 log10(mean over C,H,W of (x-y)^2 + 1e-8), at full resolution
//   SSIM  = f = max(1, round(min(H,W)/256)); f > 1: f x f average pooling (stride f, floor) of x and y;
//           11x11 gaussian window (sigma 1.5, normalised), depthwise, valid padding -> mu_x, mu_y, E[x^2], E[y^2], E[xy];
//           map = (2 mu_x mu_y + C1)/(mu_x^2 + mu_y^2 + C1) * (2 s_xy + C2)/(s_xx + s_yy + C2), C1 = 0.01^2, C2 = 0.03^2;
//           mean of the map over the channels and the (H'-10) x (W'-10) valid positions.
//
//   k_quality_tiles     grid (tiles, B*C).  A workgroup owns a QUAL_OH x QUAL_OW tile of the valid SSIM map of one channel
//                       of one frame: it stages the pooled (QUAL_OH+10) x (QUAL_OW+10) window under it in LDS (denormalise,
//                       clamp, mask and the f x f average on the way in), runs the separable window (the 2-D gaussian is the
//                       outer product of the normalised 1-D taps) horizontally and then vertically for the five moments, and
//                       sums the tile's map.  It also sums the squared error of the FULL-resolution pixels it owns: tile
//                       (ty, tx) owns rows [ty*QUAL_OH*f, (ty+1)*QUAL_OH*f) and columns likewise, the last tile of a row /
//                       column up to H / W - so the rows and columns the floor pooling drops and the border outside the
//                       valid map are counted, every pixel exactly once.  One (ssim sum, squared-error sum) pair of fp64 per
//                       (frame, channel, tile), written with plain stores.
//   k_quality_finalize  one workgroup per frame: sums its partials in a fixed order in fp64 -> psnr[b], ssim[b].
//
// No atomics: the results are bit-identical from run to run, and a frame's values do not depend on the batch it came in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rib {

#define QUAL_OW 64                   // output tile: 64 columns (one per lane of a wave) ...
#define QUAL_OH 16                   // ... by 16 rows of the valid SSIM map
#define QUAL_K 11                    // window taps
#define QUAL_WW (QUAL_OW + QUAL_K - 1)
#define QUAL_WH (QUAL_OH + QUAL_K - 1)

// exp(-(i-5)^2 / (2*1.5^2)) / sum: the normalised 1-D taps (g2d[i][j] = taps[i]*taps[j])
__constant__ float kQualTaps[QUAL_K] = {
    0.00102838008447911f, 0.007598758135239185f, 0.03600077212843083f, 0.10936068950970002f, 0.2130055377112537f,
    0.26601172486179436f, 0.2130055377112537f,   0.10936068950970002f, 0.03600077212843083f, 0.007598758135239185f,
    0.00102838008447911f};

__device__ inline float qual_unit(float v) {           // pred*std + mean, clamped to [0, 1]
  v = v * 0.5f + 0.5f;
  return fminf(fmaxf(v, 0.f), 1.f);
}

__device__ inline float qual_ssim_map(float mx, float my, float mxx, float myy, float mxy) {
  // no contraction: identical inputs must give a map of exactly 1 (mx*mx + my*my == 2*mx*my only when both are rounded)
#pragma clang fp contract(off)
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float pxx = mx * mx, pyy = my * my, pxy = mx * my;
  const float sxx = mxx - pxx, syy = myy - pyy, sxy = mxy - pxy;
  const float l = (2.f * pxy + C1) / (pxx + pyy + C1);
  const float cs = (2.f * sxy + C2) / (sxx + syy + C2);
  return l * cs;
}

__device__ inline void qual_block_sum2(double& a, double& b, double* red /* [2 * 4] */) {
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave] = a; red[4 + wave] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// partials[((b*C + c) * ntiles + tile) * 2 + {0: ssim-map sum, 1: squared-error sum}]
__global__ __launch_bounds__(256) void k_quality_tiles(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ mask, int C, int H, int W, int f, int Hp, int Wp,
                                                       int tilesX, int tilesY, double* __restrict__ partials) {
  __shared__ float sx[QUAL_WH][QUAL_WW];
  __shared__ float sy[QUAL_WH][QUAL_WW];
  __shared__ float hm[5][QUAL_WH][QUAL_OW];
  __shared__ double red[8];
  const int tid = threadIdx.x, lc = tid & 63, lr = tid >> 6;
  const int tile = blockIdx.x, tx = tile % tilesX, ty = tile / tilesX;
  const int bc = blockIdx.y, b = bc / C;
  const int ox0 = tx * QUAL_OW, oy0 = ty * QUAL_OH;           // pooled coordinates of the tile (and of its window)
  const int Hv = Hp - (QUAL_K - 1), Wv = Wp - (QUAL_K - 1);   // valid SSIM map
  const size_t plane = (size_t)H * W;
  const float* P = pred + (size_t)bc * plane;
  const float* T = target + (size_t)bc * plane;
  const float* M = mask ? mask + (size_t)b * plane : nullptr;

  // 1. the pooled window: zero outside the frame (those taps feed only outputs beyond the valid map)
  const float area = (float)(f * f);
  for (int idx = tid; idx < QUAL_WH * QUAL_WW; idx += 256) {
    const int r = idx / QUAL_WW, col = idx - r * QUAL_WW;
    const int py = oy0 + r, px = ox0 + col;
    float ax = 0.f, ay = 0.f;
    if (py < Hp && px < Wp) {
      for (int dy = 0; dy < f; ++dy) {
        const size_t row = (size_t)(py * f + dy) * W + (size_t)px * f;
        for (int dx = 0; dx < f; ++dx) {
          const float m = M ? M[row + dx] : 1.f;
          ax += qual_unit(P[row + dx]) * m;
          ay += qual_unit(T[row + dx]) * m;
        }
      }
      if (f > 1) { ax /= area; ay /= area; }
    }
    sx[r][col] = ax;
    sy[r][col] = ay;
  }
  __syncthreads();

  // 2. horizontal pass over every window row, one output column per lane
  for (int r = lr; r < QUAL_WH; r += 4) {
    float mx = 0.f, my = 0.f, mxx = 0.f, myy = 0.f, mxy = 0.f;
#pragma unroll
    for (int k = 0; k < QUAL_K; ++k) {
      const float w = kQualTaps[k], xv = sx[r][lc + k], yv = sy[r][lc + k];
      mx += w * xv; my += w * yv;
      mxx += w * (xv * xv); myy += w * (yv * yv); mxy += w * (xv * yv);
    }
    hm[0][r][lc] = mx; hm[1][r][lc] = my; hm[2][r][lc] = mxx; hm[3][r][lc] = myy; hm[4][r][lc] = mxy;
  }
  __syncthreads();

  // 3. vertical pass + the map, summed over the tile's valid positions
  double ssum = 0.0;
  for (int r = lr; r < QUAL_OH; r += 4) {
    if (oy0 + r >= Hv || ox0 + lc >= Wv) continue;
    float m5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < QUAL_K; ++k) {
      const float w = kQualTaps[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m5[q] += w * hm[q][r + k][lc];
    }
    ssum += (double)qual_ssim_map(m5[0], m5[1], m5[2], m5[3], m5[4]);
  }

  // 4. squared error of the full-resolution pixels this tile owns
  const int x0 = ox0 * f, x1 = (tx == tilesX - 1) ? W : (ox0 + QUAL_OW) * f;
  const int y0 = oy0 * f, y1 = (ty == tilesY - 1) ? H : (oy0 + QUAL_OH) * f;
  double se = 0.0;
  for (int y = y0 + lr; y < y1; y += 4) {
    float rs = 0.f;
    for (int x = x0 + lc; x < x1; x += 64) {
      const size_t o = (size_t)y * W + x;
      const float m = M ? M[o] : 1.f;
      const float d = qual_unit(P[o]) * m - qual_unit(T[o]) * m;
      rs += d * d;
    }
    se += (double)rs;
  }

  qual_block_sum2(ssum, se, red);
  if (tid == 0) {
    double* dst = partials + ((size_t)bc * tilesX * tilesY + tile) * 2;
    dst[0] = ssum;
    dst[1] = se;
  }
}

// one workgroup per frame: its C * ntiles partial pairs, summed in a fixed order
__global__ __launch_bounds__(256) void k_quality_finalize(const double* __restrict__ partials, int C, int ntiles, int H, int W,
                                                          int Hv, int Wv, float* __restrict__ psnr, float* __restrict__ ssim) {
  __shared__ double red[8];
  const int b = blockIdx.x, n = C * ntiles;
  const double* src = partials + (size_t)b * n * 2;
  double ss = 0.0, se = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) {
    ss += src[2 * j];
    se += src[2 * j + 1];
  }
  qual_block_sum2(ss, se, red);
  if (threadIdx.x == 0) {
    const double mse = se / ((double)C * H * W);
    psnr[b] = (float)(-10.0 * log10(mse + 1e-8));
    ssim[b] = (float)(ss / ((double)C * Hv * Wv));
  }
}

}  // namespace rib
