// mci.hip.h — motion-compensated interpolation of a segment's two key frames: the folder driver's background="mci" (include/rib.h:
// rib_mci_field / rib_masked_field / rib_halfpel_refine / rib_detail_field make the block field; rib_mci_frames / rib_halfpel_frames /
// rib_masked_frames / rib_scaled_frames / rib_cubic_frames / rib_cubic_scaled the frames; rib_accel_field / rib_accel_frames the
// second-order trajectory across key frames, at the end of this file).  This project's interpolation, not DAIN.
// background.py states every result in integers; every kernel here is bit-equal to it.
//
// SHARED PIECES
//   mci_luma        Y = (77 R + 150 G + 29 B + 128) >> 8: the pyramid's level 0, and what k_mci_refine and k_detail_search stage.
//   mci_valid_span  border = 1: the pixels of a block whose p - d and p + d lie inside the plane, per axis - a closed-form rectangle.
//   The frame kernels' (above k_mci_frames): mci_offsets (the two samples' offsets k D / s and (s-k) D / s; HALF: the field is in half
//   pixels, the multiplier a compile-time constant), mci_inside (VALID: a sample is valid when its position lies in [0, (H-1) << 8] x
//   [0, (W-1) << 8]), mci_blend (where exactly one of the two samples is ok the output is that sample instead of the blend),
//   mci_field_at (D(p) bilinear from the block field: exact, 1/256 px), the scaled pair's mci_scaled_pos / mci_field_row / mci_scaled_d,
//   mci_store_row (the uint8 NHWC row through LDS as 16-byte stores contiguous across the workgroup, k_panel's scheme).
//   k_scaled_frames and k_cubic_scaled are written with all of them, k_cubic_frames with offsets, blend, field_at and store_row,
//   k_mci_frames with store_row.  The three block matchers and k_mci_frames' arms are written out: profiles/r22_mci_refactor.txt.
//
// THE FIELD
//   k_mci_luma_pyramid  grid (tiles of 32 x 32, 2B): the luma of one tile and, from LDS, its 16 x 16 of level 1 and 8 x 8 of level 2
//                       ((2x2 parents, clamped, + 2) >> 2) - and, where a wider search wants them (y3, y4 not null), its 4 x 4 of
//                       level 3 and 2 x 2 of level 4: aligned tiles nest, a clamped parent is the tile's own.  Image n < B is A[n],
//                       else B[n - B].
//   k_mci_mask_pyramid  (MASKED) the same grid and tiling over the two exclusion masks [B, H, W]: level 0 as 0 / 1 and every further
//                       level as the OR of the 2x2 clamped parents, level by level through two LDS planes.
//   k_mci_search<R>     grid (runs of MCI_RUN blocks, B): bilateral block matching of one pyramid level.  A workgroup owns a run of
//                       MCI_RUN consecutive blocks; it stages, once, the two luma windows of every block - (8 + 2R)^2 bytes of A
//                       around p - start and of B around p + start, already clamped - in LDS; a wave then takes a block, its lanes
//                       the candidates (R = 4: 81 candidates, one per lane in two passes; R = 1: 9 candidates x 4 row pairs, summed
//                       over the 4 lanes by shuffles), and the winner is the wave minimum of the packed key (background.pack_key_wide:
//                       cost << 30 | dx^2 + dy^2 << 16 | dy + 128 << 8 | dx + 128, room for the +-79 of five levels): the order of
//                       the tuple (cost, |d|^2, dy, dx), whatever the lane order - and whatever the layout, so three levels give
//                       background.pack_key's winners.  No atomics.  The top level of L (3, 4 or 5) runs <MCI_TOP_R> from start 0,
//                       every level below <1>.
//     <R, VALID = true>   (background.py's border="valid") the one-sided cost at the frame border.  The staged windows are the same
//                       clamped ones; the SAD sums over the candidate's rectangle only, by a select per pixel inside the default's
//                       loops, whose bounds are uniform per block (loops from the rectangle's own, per-lane bounds took 36.8 us where
//                       these take 19.6 on level 0 of 512 x 512, B = 4: profiles/r13_mci_border.txt); n = nx * ny needs no mask and
//                       no reduction (the four row lanes of R = 1 sum their SADs and all know n), cost = 64 * SAD / n + LAMBDA's
//                       term, candidates with 4 n < N do not compete, and a block whose start itself is such a candidate (uniform
//                       per wave) stores its start.
//     <R, VALID, MASKED = true>  (the person kept out; every masked line sits under `if constexpr (MASKED)`) the two mask windows are
//                       staged beside the two luma windows (R = 4: 4 KB more per workgroup, 8.1 KB in all); a pixel counts when the
//                       border rule lets it and both mask bytes at the candidate's offsets are clear - one more term in the select,
//                       and a count n beside the SAD, summed over the row lanes of R = 1 by the same shuffles; cost = 64 * SAD / n +
//                       LAMBDA's term for either border.  The start candidate's n is one ballot (lane i takes the block's pixel i):
//                       4 n < N is uniform per wave, the block stores its start and searched = 0 and no lane reaches the shuffles.
//   k_mci_fill          (MASKED) the top level only, one thread per block: a block with searched = 0 takes the vector of the searched
//                       block within Chebyshev distance 8 that minimises (ring, |Dy| + |Dx|, Dy, Dx), ring by ring, or (0, 0).  It
//                       reads the raw field and the flags and writes ANOTHER buffer (the field the level below starts from): no
//                       thread reads what another writes, and the result does not depend on the order.
//   k_mci_median        3x3 componentwise median of the level-0 field (and of k_detail_search's), clamped.
//   k_mci_refine        (rib_halfpel_refine) one launch shaped like k_mci_search<1>: the half-pel refinement of the field after the
//                       median.  The windows are the clamped 10 x 10 INTEGER lumas of A around p - d and of B around p + d, computed
//                       from the RGB bytes while staging (no workspace); the lanes are the 9 candidates h = 2 d + e x 4 row pairs; a
//                       half-pel value is the rounded mean of the one, two or four staged integers around it (the definition's
//                       half_plane; the clamped window repeats an edge pixel where the half-pel plane is clamped, and the mean of a
//                       pixel with itself is the pixel); the winner is the wave minimum of background.pack_key_half.  <VALID = true>:
//                       the rectangle of p -+ ceil(|h| / 2).  A block reads only its own vector, staged before any is written: out
//                       may be the input.  |d| is clamped to 79 (max_disp(5)), so the key's fields always hold h.
//   k_detail_search<R>  (rib_detail_field) the same search on blocks of the FULL-SIZE frame: the comment at the kernel.
//
// THE FRAMES   grid (rows, T * B): a workgroup owns ONE row of one frame.
//   k_mci_frames<VALID, HALF, MASKED>  a thread takes 4 consecutive x: D(p), the two fixed-point bilinear samples (mci_sample), the
//                       blend; float4 stores per channel plane of the normalised NCHW tensor, and the uint8 row.  Either output may
//                       be null.  VALID: four comparisons per sample, a select.  MASKED: four byte gathers per sample in its key
//                       frame's mask (mci_clean) and one more term in the select: clean = valid under the border rule and all four
//                       taps clear; k = 0 and k = s stay A and B.
//   k_scaled_frames<VALID, HALF>  (rib_scaled_frames) k_mci_frames at the key frames' OWN size H0 x W0 - the field stays the model-size
//                       one (H x W), the samples are taken from the full-size key frames.  The row's TY, r0, r1, fy are uniform per
//                       workgroup, so the two field rows it needs are blended vertically ONCE into LDS - Wb (dx, dy) int32 pairs, at
//                       most 16 KB - and a pixel reads two of them: the definition's sum in another order.  One 32-bit division per
//                       thread for TX (mci_scaled_pos), its three further x by adding; the two 64-bit products of mci_scaled_d are
//                       the only wide arithmetic.  uint8 NHWC output only.  stage = 0 (row + field rows beyond 64 KB of LDS: both
//                       widths above 16 376): V from global.
//   k_cubic_frames, k_cubic_scaled  the same two with the 4x4 cubic sample (background.sample_cubic), a lane per pixel: the section
//                       further down says how the taps are fetched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "resize.hip.h"      // rsz_normalise: ToTensor + Normalize(0.5, 0.5) as the driver's upload computes it

namespace rib {

constexpr int MCI_BLOCK = 8, MCI_LAMBDA = 4, MCI_TOP_R = 4, MCI_KEY_BIAS = 128;     // background.py BLOCK, LAMBDA, SEARCH_TOP, WIDE_KEY_BIAS
constexpr int MCI_MIN_LEVELS = 3, MCI_MAX_LEVELS = 5;                               // background.py MIN_LEVELS, MAX_LEVELS
constexpr int MCI_RUN = 8;                  // blocks per workgroup of k_mci_search
constexpr int MCI_MAX_SIDE = 16384, MCI_MAX_RATE = 1024;
constexpr int MCI_MAX_DISP = 79, MCI_LAMBDA_HALF = 2, MCI_HALF_KEY_BIAS = 256;      // background.py max_disp(5), LAMBDA_HALF, HALF_KEY_BIAS

// luma of an RGB pixel (background.luma): the pyramid's level 0, and what k_mci_refine and k_detail_search stage
__device__ inline uint8_t mci_luma(const uint8_t* px) { return (uint8_t)((77 * px[0] + 150 * px[1] + 29 * px[2] + 128) >> 8); }

struct MciLumaParams {
  const uint8_t *a, *b;                     // [B, H, W, 3]
  uint8_t *y0, *y1, *y2, *y3, *y4;          // [2B, h_l, w_l]; y3, y4 null: not wanted (y4 only with y3)
  int B, H, W, h1, w1, h2, w2, h3, w3, h4, w4, tilesX;
};

__global__ __launch_bounds__(256) void k_mci_luma_pyramid(MciLumaParams p) {
  __shared__ uint8_t s0[32][32];
  __shared__ uint8_t s1[16][16];
  __shared__ uint8_t s2[8][8];
  __shared__ uint8_t s3[4][4];
  const int tid = threadIdx.x, n = blockIdx.y;
  const int ty = blockIdx.x / p.tilesX, tx = blockIdx.x - ty * p.tilesX;
  const uint8_t* src = (n < p.B ? p.a + (size_t)n * p.H * p.W * 3 : p.b + (size_t)(n - p.B) * p.H * p.W * 3);
  const int y00 = ty * 32, x00 = tx * 32;
  for (int i = tid; i < 1024; i += 256) {
    const int ly = i >> 5, lx = i & 31, y = y00 + ly, x = x00 + lx;
    if (y < p.H && x < p.W) {
      const uint8_t* px = src + ((size_t)y * p.W + x) * 3;
      const uint8_t v = mci_luma(px);
      s0[ly][lx] = v;
      p.y0[((size_t)n * p.H + y) * p.W + x] = v;
    }
  }
  __syncthreads();
  {
    const int ly = tid >> 4, lx = tid & 15, y = ty * 16 + ly, x = tx * 16 + lx;
    if (y < p.h1 && x < p.w1) {
      const int r0 = 2 * ly, r1 = min(2 * y + 1, p.H - 1) - y00, c0 = 2 * lx, c1 = min(2 * x + 1, p.W - 1) - x00;
      const uint8_t v = (uint8_t)((s0[r0][c0] + s0[r0][c1] + s0[r1][c0] + s0[r1][c1] + 2) >> 2);
      s1[ly][lx] = v;
      p.y1[((size_t)n * p.h1 + y) * p.w1 + x] = v;
    }
  }
  __syncthreads();
  if (tid < 64) {
    const int ly = tid >> 3, lx = tid & 7, y = ty * 8 + ly, x = tx * 8 + lx;
    if (y < p.h2 && x < p.w2) {
      const int r0 = 2 * ly, r1 = min(2 * y + 1, p.h1 - 1) - ty * 16, c0 = 2 * lx, c1 = min(2 * x + 1, p.w1 - 1) - tx * 16;
      const uint8_t v = (uint8_t)((s1[r0][c0] + s1[r0][c1] + s1[r1][c0] + s1[r1][c1] + 2) >> 2);
      s2[ly][lx] = v;
      p.y2[((size_t)n * p.h2 + y) * p.w2 + x] = v;
    }
  }
  if (!p.y3) return;                        // (uniform: three levels end here, as they always did)
  __syncthreads();
  if (tid < 16) {
    const int ly = tid >> 2, lx = tid & 3, y = ty * 4 + ly, x = tx * 4 + lx;
    if (y < p.h3 && x < p.w3) {
      const int r0 = 2 * ly, r1 = min(2 * y + 1, p.h2 - 1) - ty * 8, c0 = 2 * lx, c1 = min(2 * x + 1, p.w2 - 1) - tx * 8;
      const uint8_t v = (uint8_t)((s2[r0][c0] + s2[r0][c1] + s2[r1][c0] + s2[r1][c1] + 2) >> 2);
      s3[ly][lx] = v;
      p.y3[((size_t)n * p.h3 + y) * p.w3 + x] = v;
    }
  }
  if (!p.y4) return;
  __syncthreads();
  if (tid < 4) {
    const int ly = tid >> 1, lx = tid & 1, y = ty * 2 + ly, x = tx * 2 + lx;
    if (y < p.h4 && x < p.w4) {
      const int r0 = 2 * ly, r1 = min(2 * y + 1, p.h3 - 1) - ty * 4, c0 = 2 * lx, c1 = min(2 * x + 1, p.w3 - 1) - tx * 4;
      p.y4[((size_t)n * p.h4 + y) * p.w4 + x] = (uint8_t)((s3[r0][c0] + s3[r0][c1] + s3[r1][c0] + s3[r1][c1] + 2) >> 2);
    }
  }
}

// rib_masked_field: the OR pyramid of the two exclusion masks, k_mci_luma_pyramid's tiling with "any parent set" in place of the
// rounded mean (background.mask_pyramid).  Level 0 is stored as 0 / 1, so every reader tests one byte.
struct MciMaskParams {
  const uint8_t *ma, *mb;                   // [B, H, W], nonzero = excluded
  uint8_t* m[MCI_MAX_LEVELS];               // [2B, h_l, w_l] 0 / 1; levels beyond `levels` are not touched
  int h[MCI_MAX_LEVELS], w[MCI_MAX_LEVELS];
  int B, levels, tilesX;
};

__global__ __launch_bounds__(256) void k_mci_mask_pyramid(MciMaskParams p) {
  __shared__ uint8_t s[2][32][32];          // level l of the tile in s[l & 1], side 32 >> l
  const int tid = threadIdx.x, n = blockIdx.y;
  const int ty = blockIdx.x / p.tilesX, tx = blockIdx.x - ty * p.tilesX;
  const int H = p.h[0], W = p.w[0];
  const uint8_t* src = (n < p.B ? p.ma + (size_t)n * H * W : p.mb + (size_t)(n - p.B) * H * W);
  for (int i = tid; i < 1024; i += 256) {
    const int ly = i >> 5, lx = i & 31, y = ty * 32 + ly, x = tx * 32 + lx;
    if (y < H && x < W) {
      const uint8_t v = src[(size_t)y * W + x] != 0;
      s[0][ly][lx] = v;
      p.m[0][((size_t)n * H + y) * W + x] = v;
    }
  }
  for (int l = 1; l < p.levels; ++l) {      // (uniform: every thread reaches every barrier)
    __syncthreads();
    const int side = 32 >> l, hl = p.h[l], wl = p.w[l], hp = p.h[l - 1], wp = p.w[l - 1];
    for (int i = tid; i < side * side; i += 256) {
      const int ly = i / side, lx = i - ly * side, y = ty * side + ly, x = tx * side + lx;
      if (y < hl && x < wl) {               // aligned tiles nest: a clamped parent is the tile's own
        const int r0 = 2 * ly, r1 = min(2 * y + 1, hp - 1) - ty * 2 * side, c0 = 2 * lx, c1 = min(2 * x + 1, wp - 1) - tx * 2 * side;
        const uint8_t(*sp)[32] = s[(l - 1) & 1];
        const uint8_t v = sp[r0][c0] | sp[r0][c1] | sp[r1][c0] | sp[r1][c1];
        s[l & 1][ly][lx] = v;
        p.m[l][((size_t)n * hl + y) * wl + x] = v;
      }
    }
  }
}

struct MciSearchParams {
  const uint8_t* y;                         // [2B, h, w]: A[b] at b, B[b] at B + b
  const int16_t* coarse;                    // [B, Hbc, Wbc, 2] (dx, dy) of the coarser level, or null (start = 0)
  int16_t* out;                             // [B, Hb, Wb, 2]
  int B, h, w, Hb, Wb, Hbc, Wbc;
  const uint8_t* m;                         // <.., MASKED = true> only: [2B, h, w] 0 / 1, the level's plane of k_mci_mask_pyramid
  uint8_t* searched;                        // <.., MASKED = true> only: [B, Hb, Wb], 1 = the block's start was valid and it was searched
};

// border = 1: the pixels of the block rows / columns [o, o + len) whose p - d and p + d lie in [0, size): [lo, hi) relative to o
__device__ inline void mci_valid_span(int o, int len, int d, int size, int& lo, int& hi) {
  const int ad = abs(d);
  lo = max(ad - o, 0);
  hi = max(min(len, size - ad - o), lo);
}

template <int R, bool VALID = false, bool MASKED = false>
__global__ __launch_bounds__(256) void k_mci_search(MciSearchParams p) {
  constexpr int WS = MCI_BLOCK + 2 * R, WIN = WS * WS, SIDE = 2 * R + 1, NC = SIDE * SIDE;
  constexpr int PARTS = (NC * 4 <= 64) ? 4 : 1, ROWS = MCI_BLOCK / PARTS;
  __shared__ uint8_t s_win[MCI_RUN][2][WIN];
  __shared__ int s_start[MCI_RUN][2];
  uint8_t(*s_msk)[2][WIN] = nullptr;        // MASKED: the two mask windows beside the two luma windows (R = 4: 4 KB more, 8.1 KB in all)
  if constexpr (MASKED) {
    __shared__ uint8_t s_mwin[MCI_RUN][2][WIN];
    s_msk = s_mwin;
  }
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nblk = p.Hb * p.Wb, blk0 = blockIdx.x * MCI_RUN;
  if (tid < MCI_RUN) {
    int sx = 0, sy = 0;
    const int blk = blk0 + tid;
    if (blk < nblk && p.coarse) {
      const int by = blk / p.Wb, bx = blk - by * p.Wb;
      const int16_t* c = p.coarse + (((size_t)b * p.Hbc + min(by >> 1, p.Hbc - 1)) * p.Wbc + min(bx >> 1, p.Wbc - 1)) * 2;
      sx = 2 * c[0]; sy = 2 * c[1];
    }
    s_start[tid][0] = sx; s_start[tid][1] = sy;
  }
  __syncthreads();
  for (int i = tid; i < MCI_RUN * 2 * WIN; i += 256) {
    const int j = i / (2 * WIN), rem = i - j * 2 * WIN, which = rem / WIN, e = rem - which * WIN;
    const int wy = e / WS, wx = e - wy * WS, blk = blk0 + j;
    if (blk < nblk) {
      const int by = blk / p.Wb, bx = blk - by * p.Wb, sgn = which ? 1 : -1;
      const int y = min(max(MCI_BLOCK * by + sgn * s_start[j][1] - R + wy, 0), p.h - 1);
      const int x = min(max(MCI_BLOCK * bx + sgn * s_start[j][0] - R + wx, 0), p.w - 1);
      s_win[j][which][e] = p.y[((size_t)(which ? p.B + b : b) * p.h + y) * p.w + x];
      if constexpr (MASKED) s_msk[j][which][e] = p.m[((size_t)(which ? p.B + b : b) * p.h + y) * p.w + x];
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < MCI_RUN; j += 4) {
    const int blk = blk0 + j;
    if (blk >= nblk) break;                 // (uniform per wave; no barrier below)
    const int by = blk / p.Wb, bx = blk - by * p.Wb;
    const int ph = min(MCI_BLOCK, p.h - MCI_BLOCK * by), pw = min(MCI_BLOCK, p.w - MCI_BLOCK * bx);
    const int sx = s_start[j][0], sy = s_start[j][1];
    const uint8_t *wa = s_win[j][0], *wb = s_win[j][1];
    unsigned long long best = ~0ull;
    if constexpr (MASKED) {                 // the start candidate: lane i takes the block's pixel i, the count is a ballot
      const uint8_t *qa = s_msk[j][0], *qb = s_msk[j][1];
      const int r = lane >> 3, x = lane & 7;
      bool ok = r < ph && x < pw && !(qa[(r + R) * WS + R + x] | qb[(r + R) * WS + R + x]);
      if constexpr (VALID) {
        int xl, xh, yl, yh;
        mci_valid_span(MCI_BLOCK * bx, pw, sx, p.w, xl, xh);
        mci_valid_span(MCI_BLOCK * by, ph, sy, p.h, yl, yh);
        ok = ok && r >= yl && r < yh && x >= xl && x < xh;
      }
      const int n0 = __popcll(__ballot(ok));
      const bool go = 4 * n0 >= pw * ph;    // (uniform per wave: the shuffles below are reached by all lanes or by none)
      if (lane == 0) p.searched[(size_t)b * nblk + blk] = go;
      if (!go) {
        if (lane == 0) {
          int16_t* o = p.out + ((size_t)b * nblk + blk) * 2;
          o[0] = (int16_t)sx; o[1] = (int16_t)sy;
        }
        continue;
      }
    } else if constexpr (VALID) {           // the start candidate itself has too few valid pixels: nothing to search
      int xl, xh, yl, yh;
      mci_valid_span(MCI_BLOCK * bx, pw, sx, p.w, xl, xh);
      mci_valid_span(MCI_BLOCK * by, ph, sy, p.h, yl, yh);
      if (4 * (xh - xl) * (yh - yl) < pw * ph) {      // (uniform per wave: the shuffles below are not reached by any lane)
        if (lane == 0) {
          int16_t* o = p.out + ((size_t)b * nblk + blk) * 2;
          o[0] = (int16_t)sx; o[1] = (int16_t)sy;
        }
        continue;
      }
    }
    for (int c0 = 0; c0 < NC * PARTS; c0 += 64) {
      const int id = c0 + lane, c = id / PARTS, part = id - c * PARTS;
      const bool active = c < NC;
      const int ddy = active ? c / SIDE - R : 0, ddx = active ? c - (c / SIDE) * SIDE - R : 0;
      int sad = 0;
      int xl = 0, xh = pw, yl = 0, yh = ph;      // VALID: the candidate's rectangle, on each of its PARTS lanes
      if constexpr (VALID) {
        mci_valid_span(MCI_BLOCK * bx, pw, sx + ddx, p.w, xl, xh);
        mci_valid_span(MCI_BLOCK * by, ph, sy + ddy, p.h, yl, yh);
      }
      int n = (xh - xl) * (yh - yl);          // MASKED: counted below
      if constexpr (MASKED) n = 0;
      for (int r = part * ROWS; r < (part + 1) * ROWS; ++r) {
        if (r < ph) {
          const uint8_t* ra = wa + (r - ddy + R) * WS + (R - ddx);
          const uint8_t* rb = wb + (r + ddy + R) * WS + (R + ddx);
          if constexpr (MASKED) {             // the same offsets in the mask windows; one more term in the select, and a count
            const uint8_t* ka = s_msk[j][0] + (r - ddy + R) * WS + (R - ddx);
            const uint8_t* kb = s_msk[j][1] + (r + ddy + R) * WS + (R + ddx);
            for (int x = 0; x < pw; ++x) {
              const bool ok = !(ka[x] | kb[x]) && (!VALID || (r >= yl && r < yh && x >= xl && x < xh));
              sad += ok ? abs((int)ra[x] - (int)rb[x]) : 0;
              n += ok;
            }
          } else {
            for (int x = 0; x < pw; ++x) {
              if constexpr (VALID) sad += (r >= yl && r < yh && x >= xl && x < xh) ? abs((int)ra[x] - (int)rb[x]) : 0;
              else sad += abs((int)ra[x] - (int)rb[x]);
            }
          }
        }
      }
#pragma unroll
      for (int m = 1; m < PARTS; m <<= 1) sad += __shfl_xor(sad, m);
      if constexpr (MASKED) {
#pragma unroll
        for (int m = 1; m < PARTS; m <<= 1) n += __shfl_xor(n, m);
      }
      if constexpr (VALID || MASKED) sad = (64 * sad) / max(n, 1);      // (n = 0: not a candidate, below)
      const bool counts = (VALID || MASKED) ? active && 4 * n >= pw * ph : active;
      const int dx = sx + ddx, dy = sy + ddy;
      const unsigned long long key = ((unsigned long long)(sad + MCI_LAMBDA * (abs(dx) + abs(dy))) << 30) |
                                     ((unsigned long long)(dx * dx + dy * dy) << 16) |
                                     ((unsigned long long)((dy + MCI_KEY_BIAS) & 255) << 8) | (unsigned long long)((dx + MCI_KEY_BIAS) & 255);
      if (counts && key < best) best = key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long o = __shfl_xor(best, m);
      if (o < best) best = o;
    }
    if (lane == 0) {
      int16_t* o = p.out + ((size_t)b * nblk + blk) * 2;
      o[0] = (int16_t)((int)(best & 255) - MCI_KEY_BIAS);
      o[1] = (int16_t)((int)((best >> 8) & 255) - MCI_KEY_BIAS);
    }
  }
}

struct MciRefineParams {
  const uint8_t *a, *b;                     // [B, H, W, 3]
  const int16_t* field;                     // [B, Hb, Wb, 2] integer (dx, dy), after the median
  int16_t* out;                             // [B, Hb, Wb, 2] in half pixels; may be `field` itself
  int B, H, W, Hb, Wb;
};

// the half-pel value at offset (oy, ox) + ((fy, fx) halves) of a staged integer window: background.half_plane's rounding (a
// repeated tap gives (a + b + 1) >> 1 or the pixel itself)
__device__ inline int mci_half_tap(const uint8_t* w, int ws, int fy, int fx) {
  return (w[0] + w[fx] + w[fy * ws] + w[fy * ws + fx] + 2) >> 2;
}

template <bool VALID = false>
__global__ __launch_bounds__(256) void k_mci_refine(MciRefineParams p) {
  constexpr int R = 1, WS = MCI_BLOCK + 2 * R, WIN = WS * WS, SIDE = 3, NC = 9, PARTS = 4, ROWS = MCI_BLOCK / PARTS;
  __shared__ uint8_t s_win[MCI_RUN][2][WIN];
  __shared__ int s_start[MCI_RUN][2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nblk = p.Hb * p.Wb, blk0 = blockIdx.x * MCI_RUN;
  if (tid < MCI_RUN) {                      // a block reads its own vector only, and before any is written: in place is allowed
    int sx = 0, sy = 0;
    const int blk = blk0 + tid;
    if (blk < nblk) {
      const int16_t* c = p.field + ((size_t)b * nblk + blk) * 2;
      sx = min(max((int)c[0], -MCI_MAX_DISP), MCI_MAX_DISP); sy = min(max((int)c[1], -MCI_MAX_DISP), MCI_MAX_DISP);
    }
    s_start[tid][0] = sx; s_start[tid][1] = sy;
  }
  __syncthreads();
  for (int i = tid; i < MCI_RUN * 2 * WIN; i += 256) {
    const int j = i / (2 * WIN), rem = i - j * 2 * WIN, which = rem / WIN, e = rem - which * WIN;
    const int wy = e / WS, wx = e - wy * WS, blk = blk0 + j;
    if (blk < nblk) {
      const int by = blk / p.Wb, bx = blk - by * p.Wb, sgn = which ? 1 : -1;
      const int y = min(max(MCI_BLOCK * by + sgn * s_start[j][1] - R + wy, 0), p.H - 1);
      const int x = min(max(MCI_BLOCK * bx + sgn * s_start[j][0] - R + wx, 0), p.W - 1);
      const uint8_t* px = (which ? p.b : p.a) + (((size_t)b * p.H + y) * p.W + x) * 3;
      s_win[j][which][e] = mci_luma(px);
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < MCI_RUN; j += 4) {
    const int blk = blk0 + j;
    if (blk >= nblk) break;                 // (uniform per wave; no barrier below)
    const int by = blk / p.Wb, bx = blk - by * p.Wb;
    const int ph = min(MCI_BLOCK, p.H - MCI_BLOCK * by), pw = min(MCI_BLOCK, p.W - MCI_BLOCK * bx);
    const int sx = s_start[j][0], sy = s_start[j][1];
    const uint8_t *wa = s_win[j][0], *wb = s_win[j][1];
    int16_t* o = p.out + ((size_t)b * nblk + blk) * 2;
    if constexpr (VALID) {                  // the start 2 d keeps the pixels d keeps; too few of them: nothing to search
      int xl, xh, yl, yh;
      mci_valid_span(MCI_BLOCK * bx, pw, sx, p.W, xl, xh);
      mci_valid_span(MCI_BLOCK * by, ph, sy, p.H, yl, yh);
      if (4 * (xh - xl) * (yh - yl) < pw * ph) {      // (uniform per wave: the shuffles below are not reached by any lane)
        if (lane == 0) { o[0] = (int16_t)(2 * sx); o[1] = (int16_t)(2 * sy); }
        continue;
      }
    }
    const int c = lane / PARTS, part = lane - c * PARTS;
    const bool active = c < NC;
    const int ey = active ? c / SIDE - R : 0, ex = active ? c - (c / SIDE) * SIDE - R : 0;
    const int hx = 2 * sx + ex, hy = 2 * sy + ey;
    int xl = 0, xh = pw, yl = 0, yh = ph;
    if constexpr (VALID) {                  // 2p - h and 2p + h inside the half-pel plane: p -+ ceil(|h| / 2) inside the plane
      mci_valid_span(MCI_BLOCK * bx, pw, (abs(hx) + 1) >> 1, p.W, xl, xh);
      mci_valid_span(MCI_BLOCK * by, ph, (abs(hy) + 1) >> 1, p.H, yl, yh);
    }
    const int n = (xh - xl) * (yh - yl);
    // A at 2(p - d) - e: e = 1 starts one integer pixel lower; B at 2(p + d) + e: e = -1 does; e != 0 is a half position
    const int fy = ey != 0, fx = ex != 0;
    const int ay = R - (ey > 0), ax = R - (ex > 0), cy = R - (ey < 0), cx = R - (ex < 0);
    int sad = 0;
    for (int r = part * ROWS; r < (part + 1) * ROWS; ++r) {
      if (r < ph) {
        const uint8_t* ra = wa + (r + ay) * WS + ax;
        const uint8_t* rb = wb + (r + cy) * WS + cx;
        for (int x = 0; x < pw; ++x) {
          const int d = abs(mci_half_tap(ra + x, WS, fy, fx) - mci_half_tap(rb + x, WS, fy, fx));
          if constexpr (VALID) sad += (r >= yl && r < yh && x >= xl && x < xh) ? d : 0;
          else sad += d;
        }
      }
    }
#pragma unroll
    for (int m = 1; m < PARTS; m <<= 1) sad += __shfl_xor(sad, m);
    if constexpr (VALID) sad = (64 * sad) / max(n, 1);      // (n = 0: not a candidate, below)
    const bool counts = VALID ? active && 4 * n >= pw * ph : active;
    // background.pack_key_half: cost << 34 | hx^2 + hy^2 << 18 | hy + 256 << 9 | hx + 256
    unsigned long long best = ~0ull;
    if (counts)
      best = ((unsigned long long)(sad + MCI_LAMBDA_HALF * (abs(hx) + abs(hy))) << 34) | ((unsigned long long)(hx * hx + hy * hy) << 18) |
             ((unsigned long long)(hy + MCI_HALF_KEY_BIAS) << 9) | (unsigned long long)(hx + MCI_HALF_KEY_BIAS);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long v = __shfl_xor(best, m);
      if (v < best) best = v;
    }
    if (lane == 0) {
      o[0] = (int16_t)((int)(best & 511) - MCI_HALF_KEY_BIAS);
      o[1] = (int16_t)((int)((best >> 9) & 511) - MCI_HALF_KEY_BIAS);
    }
  }
}

// the median of nine by a fixed network of 19 compare-exchanges (statically indexed: the values stay in registers)
__device__ inline void mci_cx(int& a, int& b) { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }
__device__ inline int mci_median9(int v[9]) {
  mci_cx(v[1], v[2]); mci_cx(v[4], v[5]); mci_cx(v[7], v[8]);
  mci_cx(v[0], v[1]); mci_cx(v[3], v[4]); mci_cx(v[6], v[7]);
  mci_cx(v[1], v[2]); mci_cx(v[4], v[5]); mci_cx(v[7], v[8]);
  mci_cx(v[0], v[3]); mci_cx(v[5], v[8]); mci_cx(v[4], v[7]);
  mci_cx(v[3], v[6]); mci_cx(v[1], v[4]); mci_cx(v[2], v[5]);
  mci_cx(v[4], v[7]); mci_cx(v[4], v[2]); mci_cx(v[6], v[4]);
  mci_cx(v[4], v[2]);
  return v[4];
}

__global__ __launch_bounds__(256) void k_mci_median(const int16_t* __restrict__ in, int16_t* __restrict__ out, int B, int Hb, int Wb) {
  const int nblk = Hb * Wb;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B * nblk; i += gridDim.x * 256) {
    const int b = i / nblk, blk = i - b * nblk, by = blk / Wb, bx = blk - by * Wb;
    int vx[9], vy[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int y = min(max(by + k / 3 - 1, 0), Hb - 1), x = min(max(bx + k % 3 - 1, 0), Wb - 1);
      const int16_t* s = in + ((size_t)b * nblk + y * Wb + x) * 2;
      vx[k] = s[0]; vy[k] = s[1];
    }
    out[(size_t)i * 2] = (int16_t)mci_median9(vx);
    out[(size_t)i * 2 + 1] = (int16_t)mci_median9(vy);
  }
}

// rib_masked_field, the top level only (background.fill_unsearched): a block that was not searched takes the vector of the searched
// block within Chebyshev distance MCI_FILL_RADIUS that minimises (max(|Dy|, |Dx|), |Dy| + |Dx|, Dy, Dx), or (0, 0).  One thread per
// block, rings outwards; `in` and `out` are different buffers, so no thread reads what another writes.
constexpr int MCI_FILL_RADIUS = 8;          // background.py FILL_RADIUS

__global__ __launch_bounds__(256) void k_mci_fill(const int16_t* __restrict__ in, const uint8_t* __restrict__ searched, int16_t* __restrict__ out,
                                                  int B, int Hb, int Wb) {
  const int nblk = Hb * Wb;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B * nblk; i += gridDim.x * 256) {
    const int b = i / nblk, blk = i - b * nblk, by = blk / Wb, bx = blk - by * Wb;
    const uint8_t* flg = searched + (size_t)b * nblk;
    int src = -1;
    if (flg[blk]) src = blk;
    for (int c = 1; c <= MCI_FILL_RADIUS && src < 0; ++c) {      // ring c: the first key component; the rest by the packed minimum
      int best = INT32_MAX;
      for (int dy = -c; dy <= c; ++dy) {
        const int y = by + dy;
        if (y < 0 || y >= Hb) continue;
        const int step = (dy == -c || dy == c) ? 1 : 2 * c;      // the ring's top and bottom rows are whole, the others their two ends
        for (int dx = -c; dx <= c; dx += step) {
          const int x = bx + dx;
          if (x < 0 || x >= Wb || !flg[y * Wb + x]) continue;
          const int key = ((abs(dy) + abs(dx)) << 12) | ((dy + 32) << 6) | (dx + 32);
          best = min(best, key);
        }
      }
      if (best != INT32_MAX) src = (by + ((best >> 6) & 63) - 32) * Wb + bx + (best & 63) - 32;
    }
    int vx = 0, vy = 0;
    if (src >= 0) { const int16_t* v = in + ((size_t)b * nblk + src) * 2; vx = v[0]; vy = v[1]; }
    out[(size_t)i * 2] = (int16_t)vx;
    out[(size_t)i * 2 + 1] = (int16_t)vy;
  }
}

struct MciFramesParams {
  const uint8_t *a, *b;                     // [B, H, W, 3]
  const int16_t* field;                     // [B, Hb, Wb, 2]
  float* out_f32;                           // [T, B, 3, H, W] or null
  uint8_t* out_u8;                          // [T, B, H, W, 3] or null
  int T, B, H, W, Hb, Wb, s, ls, k_first;
  int vec;                                  // W % 4 == 0 and the outputs are aligned: float4 stores, dword LDS writes
  const uint8_t *ma, *mb;                   // <.., MASKED = true> only: [B, H, W], nonzero = excluded
};

// MASKED: the four taps of a sample's bilinear footprint in its key frame's mask are all clear (background.sample_clean;
// mci_sample's clamps)
__device__ inline bool mci_clean(const uint8_t* m, int H, int W, int py, int px) {
  const int y0 = min(max(py >> 8, 0), H - 1), y1 = min(max((py >> 8) + 1, 0), H - 1);
  const int x0 = min(max(px >> 8, 0), W - 1), x1 = min(max((px >> 8) + 1, 0), W - 1);
  return !(m[(size_t)y0 * W + x0] | m[(size_t)y0 * W + x1] | m[(size_t)y1 * W + x0] | m[(size_t)y1 * W + x1]);
}

// one bilinear sample of an RGB frame at (py, px) in 1/256 px, edge clamp (background.sample_bilinear)
__device__ inline void mci_sample(const uint8_t* img, int H, int W, int py, int px, int v[3]) {
  const int fy = py & 255, fx = px & 255;
  const int y0 = min(max(py >> 8, 0), H - 1), y1 = min(max((py >> 8) + 1, 0), H - 1);
  const int x0 = min(max(px >> 8, 0), W - 1), x1 = min(max((px >> 8) + 1, 0), W - 1);
  const uint8_t *p00 = img + ((size_t)y0 * W + x0) * 3, *p01 = img + ((size_t)y0 * W + x1) * 3;
  const uint8_t *p10 = img + ((size_t)y1 * W + x0) * 3, *p11 = img + ((size_t)y1 * W + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = ((256 - fy) * ((256 - fx) * p00[c] + fx * p01[c]) + fy * ((256 - fx) * p10[c] + fx * p11[c]) + (1 << 15)) >> 16;
}

// ---- the frame kernels' shared pieces (k_mci_frames, k_scaled_frames, k_cubic_frames, k_cubic_scaled) ----------------------------------
// the two samples' offsets from the pixel, 1/256 px: k D / s towards A and (s - k) D / s towards B, rounded; UNIT is the field's
// unit in half pixels (HALF ? 1 : 2), so the motion between the key frames is UNIT * D
template <int UNIT>
__device__ inline void mci_offsets(int Dx, int Dy, int k, int s, int ls, int& ax, int& ay, int& bx, int& by) {
  ax = (UNIT * k * Dx + (s >> 1)) >> ls; ay = (UNIT * k * Dy + (s >> 1)) >> ls;
  bx = (UNIT * (s - k) * Dx + (s >> 1)) >> ls; by = (UNIT * (s - k) * Dy + (s >> 1)) >> ls;
}

// VALID: the sample position lies in [0, (H-1) << 8] x [0, (W-1) << 8]
__device__ inline bool mci_inside(int py, int px, int H, int W) { return py >= 0 && py <= ((H - 1) << 8) && px >= 0 && px <= ((W - 1) << 8); }

// where exactly one of the two samples is ok the output is that sample, otherwise the blend (VALID's and MASKED's switch; with both
// ok known at compile time only the blend is left)
__device__ inline void mci_blend(const int v[2][3], bool oka, bool okb, int k, int s, int ls, uint8_t q[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int blend = (__mul24(s - k, v[0][c]) + __mul24(k, v[1][c]) + (s >> 1)) >> ls;      // s <= 1024, a byte: both fit 24 bits
    q[c] = (uint8_t)(oka == okb ? blend : oka ? v[0][c] : v[1][c]);
  }
}

// D(p) at the model size, bilinear from the block field in sixteenths of a block (exact, 1/256 px): rows r0, r1 and fy are the
// workgroup's, the column pair follows from x
__device__ inline void mci_field_at(const int16_t* fld, int Wb, int r0, int r1, int fy, int x, int& Dx, int& Dy) {
  const int txx = 2 * x - (MCI_BLOCK - 1), fx = txx & 15;
  const int c0 = min(max(txx >> 4, 0), Wb - 1), c1 = min(max((txx >> 4) + 1, 0), Wb - 1);
  const int16_t *f00 = fld + (r0 * Wb + c0) * 2, *f01 = fld + (r0 * Wb + c1) * 2;
  const int16_t *f10 = fld + (r1 * Wb + c0) * 2, *f11 = fld + (r1 * Wb + c1) * 2;
  Dx = (16 - fy) * ((16 - fx) * f00[0] + fx * f01[0]) + fy * ((16 - fx) * f10[0] + fx * f11[0]);
  Dy = (16 - fy) * ((16 - fx) * f00[1] + fx * f01[1]) + fy * ((16 - fx) * f10[1] + fx * f11[1]);
}

// the scaled pair (k_scaled_frames, k_cubic_scaled).  The position of output coordinate v in 1/256 block of the model's axis,
// ((2 v + 1) 16 N) // N0 - 128, would need 33 bits; it is v * qa + q0 + (v * ra + r0) // N0 with qa, ra = divmod(32 N, N0) and q0, r0 =
// divmod(16 N, N0) from the host, every term below 2^29: one 32-bit division.  rem is that division's remainder, for stepping to v + 1.
__device__ inline int mci_scaled_pos(int v, int qa, int ra, int q0, int r0, int n0, int& rem) {
  const unsigned num = (unsigned)(v * ra + r0);
  rem = (int)(num % (unsigned)n0);
  return v * qa + q0 + (int)(num / (unsigned)n0) - 128;
}
__device__ inline int mci_scaled_pos(int v, int qa, int ra, int q0, int r0, int n0) {      // where nothing steps on: TY, and k_cubic_scaled's TX
  int rem;
  return mci_scaled_pos(v, qa, ra, q0, r0, n0, rem);
}
// column c of the two field rows blended vertically ONCE, V[c] = (256-fy) f[r0][c] + fy f[r1][c] (exact: integers)
__device__ inline int2 mci_field_row(const int16_t* frow0, const int16_t* frow1, int fy, int c) {
  return make_int2((256 - fy) * frow0[2 * c] + fy * frow1[2 * c], (256 - fy) * frow0[2 * c + 1] + fy * frow1[2 * c + 1]);
}
// D16 = (256-fx) V[c0] + fx V[c1] -> D8 in 1/256 model px -> D in 1/256 output px by the 16.16 factors (the only wide arithmetic)
__device__ inline void mci_scaled_d(int2 v0, int2 v1, int fx, int sx, int sy, int& Dx, int& Dy) {
  const int D8x = ((256 - fx) * v0.x + fx * v1.x + 128) >> 8, D8y = ((256 - fx) * v0.y + fx * v1.y + 128) >> 8;
  Dx = (int)(((long long)D8x * sx + 32768) >> 16); Dy = (int)(((long long)D8y * sy + 32768) >> 16);
}

// the uint8 row from LDS as 16-byte stores contiguous across the workgroup (k_panel's scheme)
__device__ inline void mci_store_row(const uint8_t* lds, uint8_t* grow, int shift, int rowbytes) {
  const int nlines = (shift + rowbytes + 15) >> 4;
  uint8_t* gline = grow - shift;            // 16-byte aligned; only bytes [shift, shift + rowbytes) are this row's
  for (int j = threadIdx.x; j < nlines; j += 256) {
    const int lo = j * 16;
    if (lo >= shift && lo + 16 <= shift + rowbytes) {
      *reinterpret_cast<uint4*>(gline + lo) = reinterpret_cast<const uint4*>(lds)[j];
    } else {
      for (int kk = max(lo, shift); kk < min(lo + 16, shift + rowbytes); ++kk) gline[kk] = lds[kk];
    }
  }
}

template <bool VALID = false, bool HALF = false, bool MASKED = false>
__global__ __launch_bounds__(256) void k_mci_frames(MciFramesParams p) {
  constexpr int UNIT = HALF ? 1 : 2;        // the field's unit in half pixels: the motion between the key frames is UNIT * D
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mci[];
  const int y = blockIdx.x, tb = blockIdx.y, t = tb / p.B, bi = tb - t * p.B;
  const int H = p.H, W = p.W, k = p.k_first + t, s = p.s, ls = p.ls;
  const int rowbytes = W * 3;
  uint8_t* grow = p.out_u8 ? p.out_u8 + ((size_t)tb * H + y) * (size_t)rowbytes : nullptr;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_mci + shift;
  const uint8_t* A = p.a + (size_t)bi * H * W * 3;
  const uint8_t* Bf = p.b + (size_t)bi * H * W * 3;
  const int16_t* fld = p.field + (size_t)bi * p.Hb * p.Wb * 2;
  const int tyy = 2 * y - (MCI_BLOCK - 1), fy = tyy & 15;
  const int r0 = min(max(tyy >> 4, 0), p.Hb - 1), r1 = min(max((tyy >> 4) + 1, 0), p.Hb - 1);
  const size_t HW = (size_t)H * W;
  const int W4 = (W + 3) >> 2;
  for (int item = threadIdx.x; item < W4; item += 256) {
    const int x0 = item * 4;
    uint8_t q[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = min(x0 + j, W - 1);
      const int txx = 2 * x - (MCI_BLOCK - 1), fx = txx & 15;
      const int c0 = min(max(txx >> 4, 0), p.Wb - 1), c1 = min(max((txx >> 4) + 1, 0), p.Wb - 1);
      const int16_t *f00 = fld + (r0 * p.Wb + c0) * 2, *f01 = fld + (r0 * p.Wb + c1) * 2;
      const int16_t *f10 = fld + (r1 * p.Wb + c0) * 2, *f11 = fld + (r1 * p.Wb + c1) * 2;
      const int Dx = (16 - fy) * ((16 - fx) * f00[0] + fx * f01[0]) + fy * ((16 - fx) * f10[0] + fx * f11[0]);
      const int Dy = (16 - fy) * ((16 - fx) * f00[1] + fx * f01[1]) + fy * ((16 - fx) * f10[1] + fx * f11[1]);
      const int ax = (UNIT * k * Dx + (s >> 1)) >> ls, ay = (UNIT * k * Dy + (s >> 1)) >> ls;
      const int bx = (UNIT * (s - k) * Dx + (s >> 1)) >> ls, by = (UNIT * (s - k) * Dy + (s >> 1)) >> ls;
      int va[3], vb[3];
      mci_sample(A, H, W, (y << 8) - ay, (x << 8) - ax, va);
      mci_sample(Bf, H, W, (y << 8) + by, (x << 8) + bx, vb);
      if constexpr (MASKED) {                 // VALID's switch with one more condition; k = 0 and k = s stay A and B
        const int pay = (y << 8) - ay, pax = (x << 8) - ax, pby = (y << 8) + by, pbx = (x << 8) + bx;
        bool oka = mci_clean(p.ma + (size_t)bi * H * W, H, W, pay, pax), okb = mci_clean(p.mb + (size_t)bi * H * W, H, W, pby, pbx);
        if constexpr (VALID) {
          const int ymax = (H - 1) << 8, xmax = (W - 1) << 8;
          oka = oka && pay >= 0 && pay <= ymax && pax >= 0 && pax <= xmax;
          okb = okb && pby >= 0 && pby <= ymax && pbx >= 0 && pbx <= xmax;
        }
        if (k == 0) { oka = true; okb = false; }
        if (k == s) { oka = false; okb = true; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int blend = ((s - k) * va[c] + k * vb[c] + (s >> 1)) >> ls;
          q[j * 3 + c] = (uint8_t)(oka == okb ? blend : oka ? va[c] : vb[c]);
        }
      } else if constexpr (VALID) {
        const int pay = (y << 8) - ay, pax = (x << 8) - ax, pby = (y << 8) + by, pbx = (x << 8) + bx;
        const int ymax = (H - 1) << 8, xmax = (W - 1) << 8;
        const bool oka = pay >= 0 && pay <= ymax && pax >= 0 && pax <= xmax, okb = pby >= 0 && pby <= ymax && pbx >= 0 && pbx <= xmax;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int blend = ((s - k) * va[c] + k * vb[c] + (s >> 1)) >> ls;
          q[j * 3 + c] = (uint8_t)(oka == okb ? blend : oka ? va[c] : vb[c]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) q[j * 3 + c] = (uint8_t)(((s - k) * va[c] + k * vb[c] + (s >> 1)) >> ls);
      }
    }
    if (p.out_f32) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* dst = p.out_f32 + ((size_t)tb * 3 + c) * HW + (size_t)y * W + x0;
        if (p.vec) {
          *reinterpret_cast<float4*>(dst) = make_float4(rsz_normalise(q[c]), rsz_normalise(q[3 + c]), rsz_normalise(q[6 + c]), rsz_normalise(q[9 + c]));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < W) dst[j] = rsz_normalise(q[j * 3 + c]);
        }
      }
    }
    if (grow) {
      uint8_t* dst = srow + x0 * 3;
      if (p.vec) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
          reinterpret_cast<uint32_t*>(dst)[d] = (uint32_t)q[4 * d] | ((uint32_t)q[4 * d + 1] << 8) | ((uint32_t)q[4 * d + 2] << 16) | ((uint32_t)q[4 * d + 3] << 24);
      } else {
        const int nb = min(4, W - x0) * 3;
#pragma unroll
        for (int j = 0; j < 12; ++j)
          if (j < nb) dst[j] = q[j];
      }
    }
  }
  if (!grow) return;                        // (uniform: no thread reaches the barrier)
  __syncthreads();
  mci_store_row(s_mci, grow, shift, rowbytes);
}

struct ScaledFramesParams {
  const uint8_t *a, *b;                     // [B, H0, W0, 3]: the key frames at their own size
  const int16_t* field;                     // [B, Hb, Wb, 2]: the block field of the MODEL-size key frames
  uint8_t* out;                             // [T, B, H0, W0, 3]
  int T, B, H0, W0, Hb, Wb, s, ls, k_first;
  int sx, sy;                               // 16.16: (W0 * 65536 + W / 2) / W, (H0 * 65536 + H / 2) / H
  int qax, rax, q0x, r0x;                   // divmod(32 W, W0), divmod(16 W, W0)
  int qay, ray, q0y, r0y;                   // divmod(32 H, H0), divmod(16 H, H0)
  int vec;                                  // W0 % 4 == 0 and out 4-byte aligned: dword LDS writes
  int stage;                                // the blended field row fits in LDS beside the output row
  int v_off;                                // its byte offset in the dynamic LDS (a multiple of 16)
};

template <bool VALID = false, bool HALF = false>
__global__ __launch_bounds__(256) void k_scaled_frames(ScaledFramesParams p) {
  constexpr int UNIT = HALF ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mci[];
  const int y = blockIdx.x, tb = blockIdx.y, t = tb / p.B, bi = tb - t * p.B;
  const int H0 = p.H0, W0 = p.W0, k = p.k_first + t, s = p.s, ls = p.ls;
  const int rowbytes = W0 * 3;
  uint8_t* grow = p.out + ((size_t)tb * H0 + y) * (size_t)rowbytes;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_mci + shift;
  int2* sV = reinterpret_cast<int2*>(s_mci + p.v_off);
  const uint8_t* A = p.a + (size_t)bi * H0 * W0 * 3;
  const uint8_t* Bf = p.b + (size_t)bi * H0 * W0 * 3;
  const int16_t* fld = p.field + (size_t)bi * p.Hb * p.Wb * 2;
  const int tyy = mci_scaled_pos(y, p.qay, p.ray, p.q0y, p.r0y, H0), fy = tyy & 255;      // TY: y * ray + r0y < 2^28 + 2^14
  const int r0 = min(max(tyy >> 8, 0), p.Hb - 1), r1 = min(max((tyy >> 8) + 1, 0), p.Hb - 1);
  const int16_t *frow0 = fld + (size_t)r0 * p.Wb * 2, *frow1 = fld + (size_t)r1 * p.Wb * 2;
  if (p.stage) {
    for (int c = threadIdx.x; c < p.Wb; c += 256) sV[c] = mci_field_row(frow0, frow1, fy, c);
    __syncthreads();
  }
  const int W4 = (W0 + 3) >> 2;
  for (int item = threadIdx.x; item < W4; item += 256) {
    const int x0 = item * 4;
    int trem, tq = mci_scaled_pos(x0, p.qax, p.rax, p.q0x, p.r0x, W0, trem);      // TX of x0; its three further x by adding
    uint8_t q[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;                 // (x >= W0 in the last item: every index below is clamped, nothing of it is stored)
      const int fx = tq & 255;
      const int c0 = min(max(tq >> 8, 0), p.Wb - 1), c1 = min(max((tq >> 8) + 1, 0), p.Wb - 1);
      tq += p.qax; trem += p.rax;           // TX of x + 1
      if (trem >= W0) { trem -= W0; ++tq; }
      int2 v0, v1;
      if (p.stage) { v0 = sV[c0]; v1 = sV[c1]; }
      else { v0 = mci_field_row(frow0, frow1, fy, c0); v1 = mci_field_row(frow0, frow1, fy, c1); }
      int Dx, Dy, ax, ay, bx, by;
      mci_scaled_d(v0, v1, fx, p.sx, p.sy, Dx, Dy);
      mci_offsets<UNIT>(Dx, Dy, k, s, ls, ax, ay, bx, by);
      const int pay = (y << 8) - ay, pax = (x << 8) - ax, pby = (y << 8) + by, pbx = (x << 8) + bx;
      int v[2][3];
      mci_sample(A, H0, W0, pay, pax, v[0]);
      mci_sample(Bf, H0, W0, pby, pbx, v[1]);
      mci_blend(v, !VALID || mci_inside(pay, pax, H0, W0), !VALID || mci_inside(pby, pbx, H0, W0), k, s, ls, q + j * 3);
    }
    uint8_t* dst = srow + x0 * 3;           // (written out as in k_mci_frames: DESIGN.md 4g-shared)
    if (p.vec) {
#pragma unroll
      for (int d = 0; d < 3; ++d)
        reinterpret_cast<uint32_t*>(dst)[d] = (uint32_t)q[4 * d] | ((uint32_t)q[4 * d + 1] << 8) | ((uint32_t)q[4 * d + 2] << 16) | ((uint32_t)q[4 * d + 3] << 24);
    } else {
      const int nb = min(4, W0 - x0) * 3;
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < nb) dst[j] = q[j];
    }
  }
  __syncthreads();
  mci_store_row(s_mci, grow, shift, rowbytes);
}

// ---- 4x4 cubic sampling (rib_cubic_frames / rib_cubic_scaled; background.sample_cubic, the driver's mci_sampler="cubic") ------------
// k_mci_frames' and k_scaled_frames' grids (one workgroup per output row) and their shared pieces: the field arithmetic, the blend and
// border rule, the LDS scheme for the uint8 output row; what differs is the sample - 16 taps per key
// frame, Catmull-Rom weights in 1/128 per axis (background.cubic_weights) - and how the taps are fetched:
//   tile      64 consecutive x of the row, one wave, one pixel per lane (a row's tiles go round the workgroup's four waves).  Every
//             lane first has its two sample positions in registers; the wave reduces min and max of the integer tap coordinates
//             per key frame (packed int16 pairs, DPP row operations: no LDS traffic).
//   staged    both bounding boxes fit CUBIC_WIN_ROWS x CUBIC_WIN_COLS (background.cubic_tile_staged states the rule): the wave
//             copies the boxes into its own LDS windows, one RGBX dword per pixel, lanes along x so a row's loads are consecutive -
//             one dword load per pixel (the three bytes and a neighbour's, from the byte before: packed RGB has no alignment to
//             offer), clamped while staging, MASKED: the mask byte in X.  A tap is then one aligned ds_read_b32, and "all 16 taps
//             clear" is the OR of the X bytes.  Only the box is staged, not the whole window: at rest 4 x 67 pixels per key frame,
//             five loads per lane where the direct path issues 32 (a 16-bit and an 8-bit gather per tap).
//   direct    otherwise (or staging = 1): the definition, tap by tap, three byte gathers each.
//   Both paths live in one kernel and a launch mixes them tile by tile: the choice is uniform per wave, the window is the wave's
//   own (written and read by the same wave, fenced at wavefront scope), and the only workgroup barriers - after the weight table,
//   before the row's write-out - are reached by every thread.
//   weights   a 2 KB LDS table (256 x 4 int16) filled at kernel start by the integer formula of background.cubic_weights.
constexpr int CUBIC_TILE = 64, CUBIC_WIN_ROWS = 12, CUBIC_WIN_COLS = 76;      // background.py CUBIC_TILE, CUBIC_WIN_ROWS, CUBIC_WIN_COLS
constexpr int CUBIC_WIN = CUBIC_WIN_ROWS * CUBIC_WIN_COLS;                    // dwords of one key frame's window
constexpr int CUBIC_WTAB_BYTES = 256 * 4 * (int)sizeof(int16_t);
constexpr int CUBIC_WIN_BYTES = 4 * 2 * CUBIC_WIN * (int)sizeof(uint32_t);    // four waves, two key frames each: 29 184
constexpr uint32_t CUBIC_CLEAN = 0xff000000u;      // a staged or gathered tap's X byte: nonzero = excluded (MASKED), else 0

typedef short cubic_w4 __attribute__((ext_vector_type(4)));
typedef short cubic_s2 __attribute__((ext_vector_type(2)));

// background.cubic_weights' row f
__device__ inline cubic_w4 cubic_weight_row(int f) {
  const int f2 = f * f, f3 = f2 * f;
  int w0 = (-f3 + 512 * f2 - 65536 * f + (1 << 17)) >> 18;
  int w1 = (3 * f3 - 1280 * f2 + 2 * 256 * 256 * 256 + (1 << 17)) >> 18;
  int w2 = (-3 * f3 + 1024 * f2 + 65536 * f + (1 << 17)) >> 18;
  int w3 = (f3 - 256 * f2 + (1 << 17)) >> 18;
  const int rest = 128 - (w0 + w1 + w2 + w3);
  if (w1 >= w2) w1 += rest; else w2 += rest;
  cubic_w4 w;
  w.x = (short)w0; w.y = (short)w1; w.z = (short)w2; w.w = (short)w3;
  return w;
}

__device__ inline int cubic_pack(int lo, int hi) { return (int)(((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16)); }
__device__ inline int cubic_pkmin(int a, int b) {
  return __builtin_bit_cast(int, __builtin_elementwise_min(__builtin_bit_cast(cubic_s2, a), __builtin_bit_cast(cubic_s2, b)));
}
template <int CTRL, int ROWS>
__device__ inline int cubic_dpp(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false); }
// the minimum of both int16 halves over the 64 lanes of a full wave
__device__ inline int cubic_wave_pkmin(int v) {
  v = cubic_pkmin(v, cubic_dpp<0xB1, 0xf>(v));      // quad_perm:[1,0,3,2]
  v = cubic_pkmin(v, cubic_dpp<0x4E, 0xf>(v));      // quad_perm:[2,3,0,1]
  v = cubic_pkmin(v, cubic_dpp<0x141, 0xf>(v));     // row_half_mirror
  v = cubic_pkmin(v, cubic_dpp<0x140, 0xf>(v));     // row_mirror: every row of 16 holds its minimum
  v = cubic_pkmin(v, cubic_dpp<0x142, 0xa>(v));     // row_bcast:15 into rows 1 and 3
  v = cubic_pkmin(v, cubic_dpp<0x143, 0xc>(v));     // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's
  return __builtin_amdgcn_readlane(v, 63);
}

// pixel (y, x), inside the frame, as R | G << 8 | B << 16 and, MASKED, (mask != 0) << 24
template <bool MASKED>
__device__ inline uint32_t cubic_gather(const uint8_t* img, const uint8_t* msk, int W, int y, int x) {
  const int i = __mul24(y, W) + x;          // y, W <= 16384: the product fits 24-bit operands, a frame's 3 i stays below 2^30
  const uint8_t* q = img + (uint32_t)(3 * i);
  uint32_t v = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
  if constexpr (MASKED) v |= (uint32_t)(msk[i] != 0) << 24;
  return v;
}
// the same value by ONE load: the dword that starts a byte early (the frame's first pixel has no byte before it)
template <bool MASKED>
__device__ inline uint32_t cubic_load(const uint8_t* img, const uint8_t* msk, int W, int y, int x) {
  const int i = __mul24(y, W) + x;
  if (i == 0) return cubic_gather<MASKED>(img, msk, W, y, x);
  uint32_t v;
  __builtin_memcpy(&v, img + (uint32_t)(3 * i - 1), 4);
  v >>= 8;
  if constexpr (MASKED) v |= (uint32_t)(msk[i] != 0) << 24;
  return v;
}

// one tap row: acc[c] += wy * sum_j wx[j] * channel c of t[j].  Every factor fits 24 bits (|w| <= 128, a byte, |h| <= 40800): __mul24 is the
// full-rate multiply where the plain one compiled to v_mul_lo_u32, a quarter of the rate
__device__ inline void cubic_row(const uint32_t t[4], cubic_w4 wx, int wy, int acc[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int h = __mul24(wx.x, (int)((t[0] >> (8 * c)) & 255)) + __mul24(wx.y, (int)((t[1] >> (8 * c)) & 255)) +
                  __mul24(wx.z, (int)((t[2] >> (8 * c)) & 255)) + __mul24(wx.w, (int)((t[3] >> (8 * c)) & 255));
    acc[c] += __mul24(wy, h);
  }
}

struct CubicKey {                           // one key frame of one batch item
  const uint8_t *img, *msk;                 // [H, W, 3]; MASKED: [H, W], nonzero = excluded
  int py, px;                               // this lane's sample position, 1/256 px
};

// the wave's two cubic samples (background.sample_cubic) of a tile: v[f][c], and clean[f] = all 16 taps clear (MASKED).  Every
// lane of the wave is here (a lane beyond the row's end brings a neighbour's positions); `win` is this wave's 2 * CUBIC_WIN dwords,
// used when may_stage and the rule holds.
template <bool MASKED>
__device__ inline void cubic_samples(CubicKey key[2], int H, int W, bool may_stage, uint32_t* win, const cubic_w4* wtab, int lane, int v[2][3],
                                     bool clean[2]) {
  int ty[2], tx[2], lo[2], hi[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    ty[f] = key[f].py >> 8; tx[f] = key[f].px >> 8;
    lo[f] = cubic_wave_pkmin(cubic_pack(ty[f], tx[f]));
    hi[f] = cubic_wave_pkmin(cubic_pack(-ty[f], -tx[f]));
  }
  int ymin[2], xmin[2], nrows[2], ncols[2];
  bool staged = may_stage;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    ymin[f] = (int16_t)(lo[f] & 0xffff); xmin[f] = lo[f] >> 16;
    nrows[f] = -(int)(int16_t)(hi[f] & 0xffff) - ymin[f] + 4; ncols[f] = -(hi[f] >> 16) - xmin[f] + 4;
    staged = staged && nrows[f] <= CUBIC_WIN_ROWS && ncols[f] <= CUBIC_WIN_COLS;      // (uniform per wave: lo, hi are readlane results)
  }
  if (staged) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the previous tile's reads of the window are done
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int n = nrows[f] * ncols[f], inv = ((1 << 20) + ncols[f] - 1) / ncols[f];      // e / ncols = e * inv >> 20 for e < 912
      uint32_t* w = win + f * CUBIC_WIN;
      for (int e = lane; e < n; e += CUBIC_TILE) {
        const int r = __mul24(e, inv) >> 20, c = e - __mul24(r, ncols[f]);
        const int y = min(max(ymin[f] - 1 + r, 0), H - 1), x = min(max(xmin[f] - 1 + c, 0), W - 1);
        w[r * CUBIC_WIN_COLS + c] = cubic_load<MASKED>(key[f].img, key[f].msk, W, y, x);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // a lane reads what other lanes of its wave wrote
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const cubic_w4 wy = wtab[key[f].py & 255], wx = wtab[key[f].px & 255];
    const int wyr[4] = {wy.x, wy.y, wy.z, wy.w};
    int acc[3] = {0, 0, 0};
    uint32_t any = 0;
    if (staged) {
      const uint32_t* w = win + f * CUBIC_WIN + (ty[f] - ymin[f]) * CUBIC_WIN_COLS + (tx[f] - xmin[f]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t t[4] = {w[r * CUBIC_WIN_COLS], w[r * CUBIC_WIN_COLS + 1], w[r * CUBIC_WIN_COLS + 2], w[r * CUBIC_WIN_COLS + 3]};
        any |= t[0] | t[1] | t[2] | t[3];
        cubic_row(t, wx, wyr[r], acc);
      }
    } else {
      int xs[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) xs[c] = min(max(tx[f] - 1 + c, 0), W - 1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int y = min(max(ty[f] - 1 + r, 0), H - 1);
        uint32_t t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = cubic_gather<MASKED>(key[f].img, key[f].msk, W, y, xs[c]);
        any |= t[0] | t[1] | t[2] | t[3];
        cubic_row(t, wx, wyr[r], acc);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[f][c] = min(max((acc[c] + (1 << 13)) >> 14, 0), 255);
    clean[f] = !(any & CUBIC_CLEAN);
  }
}

struct CubicFramesParams {
  const uint8_t *a, *b;                     // [B, H, W, 3]
  const uint8_t *ma, *mb;                   // MASKED only: [B, H, W], nonzero = excluded
  const int16_t* field;                     // [B, Hb, Wb, 2]
  float* out_f32;                           // [T, B, 3, H, W] or null
  uint8_t* out_u8;                          // [T, B, H, W, 3] or null
  int T, B, H, W, Hb, Wb, s, ls, k_first;
  int stage;                                // 1: the windows exist and a tile that fits is staged; 0: every tile gathers (rib.h `staging` = 1)
  int w_off;                                // byte offset of the weight table in the dynamic LDS (a multiple of 16); the windows follow it
};

template <bool VALID = false, bool HALF = false, bool MASKED = false>
__global__ __launch_bounds__(256) void k_cubic_frames(CubicFramesParams p) {
  constexpr int UNIT = HALF ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mci[];
  const int y = blockIdx.x, tb = blockIdx.y, t = tb / p.B, bi = tb - t * p.B;
  const int H = p.H, W = p.W, k = p.k_first + t, s = p.s, ls = p.ls;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rowbytes = W * 3;
  uint8_t* grow = p.out_u8 ? p.out_u8 + ((size_t)tb * H + y) * (size_t)rowbytes : nullptr;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_mci + shift;
  cubic_w4* wtab = reinterpret_cast<cubic_w4*>(s_mci + p.w_off);
  uint32_t* win = reinterpret_cast<uint32_t*>(s_mci + p.w_off + CUBIC_WTAB_BYTES) + wave * 2 * CUBIC_WIN;
  wtab[threadIdx.x] = cubic_weight_row(threadIdx.x);
  __syncthreads();
  const size_t HW = (size_t)H * W;
  const uint8_t* A = p.a + (size_t)bi * HW * 3;
  const uint8_t* Bf = p.b + (size_t)bi * HW * 3;
  const uint8_t* MA = MASKED ? p.ma + (size_t)bi * HW : nullptr;
  const uint8_t* MB = MASKED ? p.mb + (size_t)bi * HW : nullptr;
  const int16_t* fld = p.field + (size_t)bi * p.Hb * p.Wb * 2;
  const int tyy = 2 * y - (MCI_BLOCK - 1), fy = tyy & 15;
  const int r0 = min(max(tyy >> 4, 0), p.Hb - 1), r1 = min(max((tyy >> 4) + 1, 0), p.Hb - 1);
  const int ntiles = (W + CUBIC_TILE - 1) / CUBIC_TILE;
  for (int tile = wave; tile < ntiles; tile += 4) {      // (uniform per wave: every lane of the wave is in cubic_samples)
    const int xo = tile * CUBIC_TILE + lane, x = min(xo, W - 1);
    int Dx, Dy, ax, ay, bx, by;
    mci_field_at(fld, p.Wb, r0, r1, fy, x, Dx, Dy);
    mci_offsets<UNIT>(Dx, Dy, k, s, ls, ax, ay, bx, by);
    CubicKey key[2] = {{A, MA, (y << 8) - ay, (x << 8) - ax}, {Bf, MB, (y << 8) + by, (x << 8) + bx}};
    int v[2][3];
    bool ok[2];
    cubic_samples<MASKED>(key, H, W, p.stage != 0, win, wtab, lane, v, ok);
    if constexpr (VALID) {
      const int ymax = (H - 1) << 8, xmax = (W - 1) << 8;
#pragma unroll
      for (int f = 0; f < 2; ++f) ok[f] = ok[f] && key[f].py >= 0 && key[f].py <= ymax && key[f].px >= 0 && key[f].px <= xmax;
    }
    if constexpr (MASKED) {                 // k = 0 and k = s stay A and B
      if (k == 0) { ok[0] = true; ok[1] = false; }
      if (k == s) { ok[0] = false; ok[1] = true; }
    }
    uint8_t q[3];
    mci_blend(v, ok[0], ok[1], k, s, ls, q);
    if (xo < W) {
      if (p.out_f32) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out_f32[((size_t)tb * 3 + c) * HW + (size_t)y * W + xo] = rsz_normalise(q[c]);
      }
      if (grow) {
#pragma unroll
        for (int c = 0; c < 3; ++c) srow[xo * 3 + c] = q[c];
      }
    }
  }
  if (!grow) return;                        // (uniform: no thread reaches the barrier)
  __syncthreads();
  mci_store_row(s_mci, grow, shift, rowbytes);
}

struct CubicScaledParams {
  ScaledFramesParams f;                     // k_scaled_frames' own (vec is not used: a lane writes one pixel)
  int stage_win;                            // CubicFramesParams::stage
  int w_off;                                // byte offset of the weight table in the dynamic LDS; the windows follow it
};

template <bool VALID = false, bool HALF = false>
__global__ __launch_bounds__(256) void k_cubic_scaled(CubicScaledParams cp) {
  constexpr int UNIT = HALF ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mci[];
  const ScaledFramesParams& p = cp.f;
  const int y = blockIdx.x, tb = blockIdx.y, t = tb / p.B, bi = tb - t * p.B;
  const int H0 = p.H0, W0 = p.W0, k = p.k_first + t, s = p.s, ls = p.ls;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rowbytes = W0 * 3;
  uint8_t* grow = p.out + ((size_t)tb * H0 + y) * (size_t)rowbytes;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_mci + shift;
  int2* sV = reinterpret_cast<int2*>(s_mci + p.v_off);
  cubic_w4* wtab = reinterpret_cast<cubic_w4*>(s_mci + cp.w_off);
  uint32_t* win = reinterpret_cast<uint32_t*>(s_mci + cp.w_off + CUBIC_WTAB_BYTES) + wave * 2 * CUBIC_WIN;
  const uint8_t* A = p.a + (size_t)bi * H0 * W0 * 3;
  const uint8_t* Bf = p.b + (size_t)bi * H0 * W0 * 3;
  const int16_t* fld = p.field + (size_t)bi * p.Hb * p.Wb * 2;
  const int tyy = mci_scaled_pos(y, p.qay, p.ray, p.q0y, p.r0y, H0), fy = tyy & 255;
  const int r0 = min(max(tyy >> 8, 0), p.Hb - 1), r1 = min(max((tyy >> 8) + 1, 0), p.Hb - 1);
  const int16_t *frow0 = fld + (size_t)r0 * p.Wb * 2, *frow1 = fld + (size_t)r1 * p.Wb * 2;
  wtab[threadIdx.x] = cubic_weight_row(threadIdx.x);
  for (int c = threadIdx.x; c < p.Wb; c += 256) sV[c] = mci_field_row(frow0, frow1, fy, c);      // it always has room (the host raises the kernel's LDS limit)
  __syncthreads();
  const int ntiles = (W0 + CUBIC_TILE - 1) / CUBIC_TILE;
  for (int tile = wave; tile < ntiles; tile += 4) {      // (uniform per wave)
    const int xo = tile * CUBIC_TILE + lane, x = min(xo, W0 - 1);
    const int tq = mci_scaled_pos(x, p.qax, p.rax, p.q0x, p.r0x, W0), fx = tq & 255;      // (a lane takes one x: nothing to step)
    const int c0 = min(max(tq >> 8, 0), p.Wb - 1), c1 = min(max((tq >> 8) + 1, 0), p.Wb - 1);
    int Dx, Dy, ax, ay, bx, by;
    mci_scaled_d(sV[c0], sV[c1], fx, p.sx, p.sy, Dx, Dy);
    mci_offsets<UNIT>(Dx, Dy, k, s, ls, ax, ay, bx, by);
    CubicKey key[2] = {{A, nullptr, (y << 8) - ay, (x << 8) - ax}, {Bf, nullptr, (y << 8) + by, (x << 8) + bx}};
    int v[2][3];
    bool ok[2];
    cubic_samples<false>(key, H0, W0, cp.stage_win != 0, win, wtab, lane, v, ok);
    if constexpr (VALID) {
#pragma unroll
      for (int f = 0; f < 2; ++f) ok[f] = mci_inside(key[f].py, key[f].px, H0, W0);
    }
    uint8_t q[3];
    mci_blend(v, ok[0], ok[1], k, s, ls, q);
    if (xo < W0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) srow[xo * 3 + c] = q[c];
    }
  }
  __syncthreads();
  mci_store_row(s_mci, grow, shift, rowbytes);
}

// ---- the field refined at the key frames' own size (rib_detail_field; background.mci_detail_field_host, the driver's mci_detail="keyframes") ----
// k_detail_search<R>  grid (runs of MCI_RUN blocks of the FULL-SIZE frame, B), shaped like k_mci_search and k_mci_refine.  A workgroup
//                     owns a run of MCI_RUN blocks; thread j < MCI_RUN computes block j's start itself - background.detail_start: the
//                     bilinear model-size field at the block's pixel (min(8 by + 4, H0 - 1), min(8 bx + 4, W0 - 1)) from its four
//                     vectors, D8 = (D16 + 128) >> 8, DS = (D8 * S + 32768) >> 16 (64-bit product, 16.16 factors from the host),
//                     start = (DS + 128) >> 8, or (DS + 256) >> 9 where the field is in half pixels - so there is no start launch and
//                     no start buffer; the two clamped (8 + 2R)^2 windows of A around p - start and of B around p + start are staged as
//                     luma computed from the RGB bytes while staging (no full-size luma plane); a wave takes a block, its lanes the
//                     candidates times PARTS row parts (R = 1: 9 x 4, R = 2: 25 x 2, R = 3: 49, R = 4: 81 in two passes); the winner is
//                     the wave minimum, by shuffles, of background.pack_key_detail: cost << 46 | dx^2 + dy^2 << 24 | dy + 2048 << 12 |
//                     dx + 2048 - the tuple's order with room for |d| <= 79 * 16 + 4 = 1268.  <R, VALID = true>: k_mci_search's
//                     rectangle, 64 * SAD / n, 4 n >= N, and a block whose start is not valid stores its start.  No atomics, nothing of
//                     another block read or written: independent of B.  The model-size vectors are clamped to +-79 (+-159 in half
//                     pixels), so the key's fields always hold d; every staged coordinate is clamped to the frame.
//                     k_mci_median follows, as it is.
constexpr int DETAIL_KEY_BIAS = 2048, DETAIL_MAX_R = 4;      // background.py DETAIL_KEY_BIAS, DETAIL_MAX_RADIUS

struct DetailSearchParams {
  const uint8_t *a, *b;                     // [B, H0, W0, 3]: the key frames at their own size
  const int16_t* field;                     // [B, Hb, Wb, 2]: the block field of the MODEL-size key frames
  int16_t* out;                             // [B, H0b, W0b, 2] in whole output pixels, before the median
  int B, H, W, H0, W0, Hb, Wb, H0b, W0b;
  int sx, sy;                               // 16.16: (W0 * 65536 + W / 2) / W, (H0 * 65536 + H / 2) / H
  int half;                                 // the field is in half pixels
};

// background.pixel_field_scaled's position of output coordinate v (of n0) in 1/256 block of the model's axis (n): 64-bit, once per block
__device__ inline int detail_pos(int v, int n, int n0) { return (int)(((long long)(2 * v + 1) * n * 16) / n0) - 128; }

template <int R, bool VALID = false>
__global__ __launch_bounds__(256) void k_detail_search(DetailSearchParams p) {
  constexpr int WS = MCI_BLOCK + 2 * R, WIN = WS * WS, SIDE = 2 * R + 1, NC = SIDE * SIDE;
  constexpr int PARTS = (NC * 4 <= 64) ? 4 : (NC * 2 <= 64) ? 2 : 1, ROWS = MCI_BLOCK / PARTS;
  __shared__ uint8_t s_win[MCI_RUN][2][WIN];
  __shared__ int s_start[MCI_RUN][2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nblk = p.H0b * p.W0b, blk0 = blockIdx.x * MCI_RUN;
  if (tid < MCI_RUN) {
    int sx = 0, sy = 0;
    const int blk = blk0 + tid;
    if (blk < nblk) {
      const int by = blk / p.W0b, bx = blk - by * p.W0b;
      const int ty = detail_pos(min(MCI_BLOCK * by + 4, p.H0 - 1), p.H, p.H0), tx = detail_pos(min(MCI_BLOCK * bx + 4, p.W0 - 1), p.W, p.W0);
      const int fy = ty & 255, fx = tx & 255;
      const int r0 = min(max(ty >> 8, 0), p.Hb - 1), r1 = min(max((ty >> 8) + 1, 0), p.Hb - 1);
      const int c0 = min(max(tx >> 8, 0), p.Wb - 1), c1 = min(max((tx >> 8) + 1, 0), p.Wb - 1);
      const int16_t* f = p.field + (size_t)b * p.Hb * p.Wb * 2;
      const int lim = p.half ? 2 * MCI_MAX_DISP + 1 : MCI_MAX_DISP;
      int d[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int f00 = min(max((int)f[(r0 * p.Wb + c0) * 2 + c], -lim), lim), f01 = min(max((int)f[(r0 * p.Wb + c1) * 2 + c], -lim), lim);
        const int f10 = min(max((int)f[(r1 * p.Wb + c0) * 2 + c], -lim), lim), f11 = min(max((int)f[(r1 * p.Wb + c1) * 2 + c], -lim), lim);
        const int d16 = (256 - fy) * ((256 - fx) * f00 + fx * f01) + fy * ((256 - fx) * f10 + fx * f11);
        const int d8 = (d16 + 128) >> 8;                                                        // 1/256 model px
        const int ds = (int)(((long long)d8 * (c ? p.sy : p.sx) + 32768) >> 16);               // 1/256 output px
        d[c] = p.half ? (ds + 256) >> 9 : (ds + 128) >> 8;
      }
      sx = d[0]; sy = d[1];
    }
    s_start[tid][0] = sx; s_start[tid][1] = sy;
  }
  __syncthreads();
  for (int i = tid; i < MCI_RUN * 2 * WIN; i += 256) {
    const int j = i / (2 * WIN), rem = i - j * 2 * WIN, which = rem / WIN, e = rem - which * WIN;
    const int wy = e / WS, wx = e - wy * WS, blk = blk0 + j;
    if (blk < nblk) {
      const int by = blk / p.W0b, bx = blk - by * p.W0b, sgn = which ? 1 : -1;
      const int y = min(max(MCI_BLOCK * by + sgn * s_start[j][1] - R + wy, 0), p.H0 - 1);
      const int x = min(max(MCI_BLOCK * bx + sgn * s_start[j][0] - R + wx, 0), p.W0 - 1);
      const uint8_t* px = (which ? p.b : p.a) + (((size_t)b * p.H0 + y) * p.W0 + x) * 3;
      s_win[j][which][e] = mci_luma(px);
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < MCI_RUN; j += 4) {
    const int blk = blk0 + j;
    if (blk >= nblk) break;                 // (uniform per wave; no barrier below)
    const int by = blk / p.W0b, bx = blk - by * p.W0b;
    const int ph = min(MCI_BLOCK, p.H0 - MCI_BLOCK * by), pw = min(MCI_BLOCK, p.W0 - MCI_BLOCK * bx);
    const int sx = s_start[j][0], sy = s_start[j][1];
    const uint8_t *wa = s_win[j][0], *wb = s_win[j][1];
    int16_t* o = p.out + ((size_t)b * nblk + blk) * 2;
    if constexpr (VALID) {                  // the start candidate itself has too few valid pixels: nothing to search
      int xl, xh, yl, yh;
      mci_valid_span(MCI_BLOCK * bx, pw, sx, p.W0, xl, xh);
      mci_valid_span(MCI_BLOCK * by, ph, sy, p.H0, yl, yh);
      if (4 * (xh - xl) * (yh - yl) < pw * ph) {      // (uniform per wave: the shuffles below are not reached by any lane)
        if (lane == 0) { o[0] = (int16_t)sx; o[1] = (int16_t)sy; }
        continue;
      }
    }
    unsigned long long best = ~0ull;
    for (int c0 = 0; c0 < NC * PARTS; c0 += 64) {
      const int id = c0 + lane, c = id / PARTS, part = id - c * PARTS;
      const bool active = c < NC;
      const int ddy = active ? c / SIDE - R : 0, ddx = active ? c - (c / SIDE) * SIDE - R : 0;
      int xl = 0, xh = pw, yl = 0, yh = ph;      // VALID: the candidate's rectangle, on each of its PARTS lanes
      if constexpr (VALID) {
        mci_valid_span(MCI_BLOCK * bx, pw, sx + ddx, p.W0, xl, xh);
        mci_valid_span(MCI_BLOCK * by, ph, sy + ddy, p.H0, yl, yh);
      }
      const int n = (xh - xl) * (yh - yl);
      int sad = 0;
      for (int r = part * ROWS; r < (part + 1) * ROWS; ++r) {
        if (r < ph) {
          const uint8_t* ra = wa + (r - ddy + R) * WS + (R - ddx);
          const uint8_t* rb = wb + (r + ddy + R) * WS + (R + ddx);
          for (int x = 0; x < pw; ++x) {
            if constexpr (VALID) sad += (r >= yl && r < yh && x >= xl && x < xh) ? abs((int)ra[x] - (int)rb[x]) : 0;
            else sad += abs((int)ra[x] - (int)rb[x]);
          }
        }
      }
#pragma unroll
      for (int m = 1; m < PARTS; m <<= 1) sad += __shfl_xor(sad, m);
      if constexpr (VALID) sad = (64 * sad) / max(n, 1);      // (n = 0: not a candidate, below)
      const bool counts = VALID ? active && 4 * n >= pw * ph : active;
      const int dx = sx + ddx, dy = sy + ddy;
      const unsigned long long key = ((unsigned long long)(sad + MCI_LAMBDA * (abs(dx) + abs(dy))) << 46) | ((unsigned long long)(dx * dx + dy * dy) << 24) |
                                     ((unsigned long long)(dy + DETAIL_KEY_BIAS) << 12) | (unsigned long long)(dx + DETAIL_KEY_BIAS);
      if (counts && key < best) best = key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long v = __shfl_xor(best, m);
      if (v < best) best = v;
    }
    if (lane == 0) {
      o[0] = (int16_t)((int)(best & 4095) - DETAIL_KEY_BIAS);
      o[1] = (int16_t)((int)((best >> 12) & 4095) - DETAIL_KEY_BIAS);
    }
  }
}

// ---- quadratic motion across key frames (rib_accel_field / rib_accel_frames; background.mci_accel_host / mci_frames_accel_host, the
// driver's mci_motion="quadratic") -------------------------------------------------------------------------------------------------
// k_mci_accel         one thread per block of one segment (a flat grid over B * Hb * Wb, as k_mci_median's): the block's own vector in
//                     whole pixels (a half-pel field shifted with floor), the previous segment's field read at the block two vectors
//                     back, the next one's two vectors on (block coordinates clamped), a = next - prev, or twice the one-sided
//                     difference to the block's own vector where one neighbour is missing, or 0: the field BEFORE the median;
//                     k_mci_median follows, as it is.  prev / next null: no item has that neighbour; present [B, 2] (prev, next)
//                     bytes: per item, for groups whose members differ.  Every index is clamped; nothing of `out` is read.
// k_accel_frames<VALID, HALF, MASKED>, k_cubic_accel<VALID, HALF, MASKED>
//                     k_mci_frames' and k_cubic_frames' grids, outputs and LDS schemes, written with the shared pieces; per pixel one
//                     more mci_field_at in the acceleration field and mci_accel_c: BOTH sample positions move by c = UNIT k (s - k)
//                     Acc / (4 s^2), rounded, a 64-bit product.  The cubic tile's staging rule (cubic_samples) sees the corrected
//                     positions.  They are kernels of their own so that k_mci_frames and k_cubic_frames keep their instruction streams.
struct MciAccelParams {
  const int16_t *prev, *cur, *next;         // [B, Hb, Wb, 2]; prev, next may be null
  const uint8_t* present;                   // [B, 2] (prev, next) nonzero = this item has it, or null: every item has what is not null
  int16_t* out;                             // [B, Hb, Wb, 2] before the median
  int B, Hb, Wb, shift;                     // shift: 1 = the fields are in half pixels
};

__global__ __launch_bounds__(256) void k_mci_accel(MciAccelParams p) {
  const int nblk = p.Hb * p.Wb;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < p.B * nblk; i += gridDim.x * 256) {
    const int b = i / nblk, blk = i - b * nblk, by = blk / p.Wb, bx = blk - by * p.Wb;
    const size_t item = (size_t)b * nblk;
    const int fx = p.cur[(item + blk) * 2], fy = p.cur[(item + blk) * 2 + 1];
    const int wx = fx >> p.shift, wy = fy >> p.shift;
    const bool hp = p.prev && (!p.present || p.present[2 * b]), hn = p.next && (!p.present || p.present[2 * b + 1]);
    int px = fx, py = fy, nx = fx, ny = fy;   // a missing side stands in as the block's own vector: the one-sided difference
    if (hp) {
      const int y = min(max((MCI_BLOCK * by + 4 - 2 * wy) >> 3, 0), p.Hb - 1), x = min(max((MCI_BLOCK * bx + 4 - 2 * wx) >> 3, 0), p.Wb - 1);
      const int16_t* s = p.prev + (item + y * p.Wb + x) * 2;
      px = s[0]; py = s[1];
    }
    if (hn) {
      const int y = min(max((MCI_BLOCK * by + 4 + 2 * wy) >> 3, 0), p.Hb - 1), x = min(max((MCI_BLOCK * bx + 4 + 2 * wx) >> 3, 0), p.Wb - 1);
      const int16_t* s = p.next + (item + y * p.Wb + x) * 2;
      nx = s[0]; ny = s[1];
    }
    const int m = hp && hn ? 1 : 2;           // (neither: next - prev is 0 already)
    p.out[(item + blk) * 2] = (int16_t)(m * (nx - px));
    p.out[(item + blk) * 2 + 1] = (int16_t)(m * (ny - py));
  }
}

// c of one component: (m * Acc + 2 s^2) >> (2 log2 s + 2) with m = UNIT * k * (s - k) <= 2^19 and Acc in 1/256 of the field's unit
// (|Acc| < 2^23): the product needs 64 bits from s = 64 on
__device__ inline int mci_accel_c(int Acc, int m, int ls) { return (int)(((long long)m * Acc + (2ll << (2 * ls))) >> (2 * ls + 2)); }

struct AccelFramesParams {
  MciFramesParams f;                        // k_mci_frames' own
  const int16_t* accel;                     // [B, Hb, Wb, 2]: k_mci_accel's field after the median, in the field's unit
};

template <bool VALID = false, bool HALF = false, bool MASKED = false>
__global__ __launch_bounds__(256) void k_accel_frames(AccelFramesParams ap) {
  constexpr int UNIT = HALF ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mci[];
  const MciFramesParams& p = ap.f;
  const int y = blockIdx.x, tb = blockIdx.y, t = tb / p.B, bi = tb - t * p.B;
  const int H = p.H, W = p.W, k = p.k_first + t, s = p.s, ls = p.ls;
  const int rowbytes = W * 3;
  uint8_t* grow = p.out_u8 ? p.out_u8 + ((size_t)tb * H + y) * (size_t)rowbytes : nullptr;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_mci + shift;
  const size_t HW = (size_t)H * W;
  const uint8_t* A = p.a + (size_t)bi * HW * 3;
  const uint8_t* Bf = p.b + (size_t)bi * HW * 3;
  const int16_t* fld = p.field + (size_t)bi * p.Hb * p.Wb * 2;
  const int16_t* acc = ap.accel + (size_t)bi * p.Hb * p.Wb * 2;
  const int tyy = 2 * y - (MCI_BLOCK - 1), fy = tyy & 15;
  const int r0 = min(max(tyy >> 4, 0), p.Hb - 1), r1 = min(max((tyy >> 4) + 1, 0), p.Hb - 1);
  const int m = UNIT * k * (s - k);
  const int W4 = (W + 3) >> 2;
  for (int item = threadIdx.x; item < W4; item += 256) {
    const int x0 = item * 4;
    uint8_t q[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = min(x0 + j, W - 1);
      int Dx, Dy, Ax, Ay, ax, ay, bx, by;
      mci_field_at(fld, p.Wb, r0, r1, fy, x, Dx, Dy);
      mci_field_at(acc, p.Wb, r0, r1, fy, x, Ax, Ay);
      mci_offsets<UNIT>(Dx, Dy, k, s, ls, ax, ay, bx, by);
      const int cx = mci_accel_c(Ax, m, ls), cy = mci_accel_c(Ay, m, ls);
      const int pay = (y << 8) - ay + cy, pax = (x << 8) - ax + cx, pby = (y << 8) + by + cy, pbx = (x << 8) + bx + cx;
      int v[2][3];
      mci_sample(A, H, W, pay, pax, v[0]);
      mci_sample(Bf, H, W, pby, pbx, v[1]);
      bool oka = !VALID || mci_inside(pay, pax, H, W), okb = !VALID || mci_inside(pby, pbx, H, W);
      if constexpr (MASKED) {                 // clean = valid under the border rule and all four taps clear; k = 0 and k = s stay A and B
        oka = oka && mci_clean(p.ma + (size_t)bi * HW, H, W, pay, pax);
        okb = okb && mci_clean(p.mb + (size_t)bi * HW, H, W, pby, pbx);
        if (k == 0) { oka = true; okb = false; }
        if (k == s) { oka = false; okb = true; }
      }
      mci_blend(v, oka, okb, k, s, ls, q + j * 3);
    }
    if (p.out_f32) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* dst = p.out_f32 + ((size_t)tb * 3 + c) * HW + (size_t)y * W + x0;
        if (p.vec) {
          *reinterpret_cast<float4*>(dst) = make_float4(rsz_normalise(q[c]), rsz_normalise(q[3 + c]), rsz_normalise(q[6 + c]), rsz_normalise(q[9 + c]));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (x0 + j < W) dst[j] = rsz_normalise(q[j * 3 + c]);
        }
      }
    }
    if (grow) {                             // (written out as in k_mci_frames: DESIGN.md 4g-shared)
      uint8_t* dst = srow + x0 * 3;
      if (p.vec) {
#pragma unroll
        for (int d = 0; d < 3; ++d)
          reinterpret_cast<uint32_t*>(dst)[d] = (uint32_t)q[4 * d] | ((uint32_t)q[4 * d + 1] << 8) | ((uint32_t)q[4 * d + 2] << 16) | ((uint32_t)q[4 * d + 3] << 24);
      } else {
        const int nb = min(4, W - x0) * 3;
#pragma unroll
        for (int j = 0; j < 12; ++j)
          if (j < nb) dst[j] = q[j];
      }
    }
  }
  if (!grow) return;                        // (uniform: no thread reaches the barrier)
  __syncthreads();
  mci_store_row(s_mci, grow, shift, rowbytes);
}

struct CubicAccelParams {
  CubicFramesParams f;                      // k_cubic_frames' own
  const int16_t* accel;                     // [B, Hb, Wb, 2]
};

template <bool VALID = false, bool HALF = false, bool MASKED = false>
__global__ __launch_bounds__(256) void k_cubic_accel(CubicAccelParams ap) {
  constexpr int UNIT = HALF ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mci[];
  const CubicFramesParams& p = ap.f;
  const int y = blockIdx.x, tb = blockIdx.y, t = tb / p.B, bi = tb - t * p.B;
  const int H = p.H, W = p.W, k = p.k_first + t, s = p.s, ls = p.ls;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rowbytes = W * 3;
  uint8_t* grow = p.out_u8 ? p.out_u8 + ((size_t)tb * H + y) * (size_t)rowbytes : nullptr;
  const int shift = (int)(reinterpret_cast<uintptr_t>(grow) & 15);
  uint8_t* srow = s_mci + shift;
  cubic_w4* wtab = reinterpret_cast<cubic_w4*>(s_mci + p.w_off);
  uint32_t* win = reinterpret_cast<uint32_t*>(s_mci + p.w_off + CUBIC_WTAB_BYTES) + wave * 2 * CUBIC_WIN;
  wtab[threadIdx.x] = cubic_weight_row(threadIdx.x);
  __syncthreads();
  const size_t HW = (size_t)H * W;
  const uint8_t* A = p.a + (size_t)bi * HW * 3;
  const uint8_t* Bf = p.b + (size_t)bi * HW * 3;
  const uint8_t* MA = MASKED ? p.ma + (size_t)bi * HW : nullptr;
  const uint8_t* MB = MASKED ? p.mb + (size_t)bi * HW : nullptr;
  const int16_t* fld = p.field + (size_t)bi * p.Hb * p.Wb * 2;
  const int16_t* acc = ap.accel + (size_t)bi * p.Hb * p.Wb * 2;
  const int tyy = 2 * y - (MCI_BLOCK - 1), fy = tyy & 15;
  const int r0 = min(max(tyy >> 4, 0), p.Hb - 1), r1 = min(max((tyy >> 4) + 1, 0), p.Hb - 1);
  const int m = UNIT * k * (s - k);
  const int ntiles = (W + CUBIC_TILE - 1) / CUBIC_TILE;
  for (int tile = wave; tile < ntiles; tile += 4) {      // (uniform per wave: every lane of the wave is in cubic_samples)
    const int xo = tile * CUBIC_TILE + lane, x = min(xo, W - 1);
    int Dx, Dy, Ax, Ay, ax, ay, bx, by;
    mci_field_at(fld, p.Wb, r0, r1, fy, x, Dx, Dy);
    mci_field_at(acc, p.Wb, r0, r1, fy, x, Ax, Ay);
    mci_offsets<UNIT>(Dx, Dy, k, s, ls, ax, ay, bx, by);
    const int cx = mci_accel_c(Ax, m, ls), cy = mci_accel_c(Ay, m, ls);
    CubicKey key[2] = {{A, MA, (y << 8) - ay + cy, (x << 8) - ax + cx}, {Bf, MB, (y << 8) + by + cy, (x << 8) + bx + cx}};
    int v[2][3];
    bool ok[2];
    cubic_samples<MASKED>(key, H, W, p.stage != 0, win, wtab, lane, v, ok);
    if constexpr (VALID) {
#pragma unroll
      for (int f = 0; f < 2; ++f) ok[f] = ok[f] && mci_inside(key[f].py, key[f].px, H, W);
    }
    if constexpr (MASKED) {                 // k = 0 and k = s stay A and B
      if (k == 0) { ok[0] = true; ok[1] = false; }
      if (k == s) { ok[0] = false; ok[1] = true; }
    }
    uint8_t q[3];
    mci_blend(v, ok[0], ok[1], k, s, ls, q);
    if (xo < W) {
      if (p.out_f32) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out_f32[((size_t)tb * 3 + c) * HW + (size_t)y * W + xo] = rsz_normalise(q[c]);
      }
      if (grow) {
#pragma unroll
        for (int c = 0; c < 3; ++c) srow[xo * 3 + c] = q[c];
      }
    }
  }
  if (!grow) return;                        // (uniform: no thread reaches the barrier)
  __syncthreads();
  mci_store_row(s_mci, grow, shift, rowbytes);
}

}  // namespace rib
