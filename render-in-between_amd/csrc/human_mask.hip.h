// human_mask.hip.h — the human-centric mask of the ground-truth metrics, drawn on the GPU.
//
// The reference measures PSNR / SSIM under the mask _generate_human_mask draws from the frame's own keypoints
// (PGNR/datasets/HSM_auto_dataset.py:254-334, used at :390; PGNR/models/evaluator.py:118,122): cv2.circle (filled) on every
// valid joint, radius 30 on joint 0 and 15 elsewhere, and cv2.line on every limb whose two joints are valid, thickness 30
// (head, arms, legs) or 40 (the three body lines).  Restated from OpenCV's drawing, unpinned (cv2 is not in this image); the
// definition is rasterise.human_mask's, in integers only, so host and device agree bit for bit by construction:
//
//   disc(P, R)      (px-Px)^2 + (py-Py)^2 <= R*R + R                  every valid joint; both ends of every drawn limb, R = t/2
//   slab(A, B, h)   d = B-A, L2 = d.d, v = (px,py)-A:  0 <= v.d <= L2  and  4 (vx dy - vy dx)^2 <= (2h+1)^2 L2,   A != B, h = t/2
//
// A pixel is set iff one test holds: a union, so - unlike k_skeleton - nothing is sequential.  With H, W <= 16384 every
// difference is below 2^14, every dot / cross product below 2^29 (int32); only the squared, scaled comparison is 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rib {

constexpr int HMASK_TW = 64, HMASK_TH = 16;      // tile of one workgroup: 16 lanes x 4 pixels wide, 16 rows
constexpr int HMASK_MAXJ = 19, HMASK_NLIMBS = 20;      // 16 limbs of every pose + 4 of a 19-joint pose
constexpr int HMASK_MAX_SIDE = 16384;

// (joint a, joint b, thickness) in the reference's order: head, hand, legs, body, then the four limbs of a 19-joint pose
__device__ constexpr uint8_t kMaskLimbs[HMASK_NLIMBS][3] = {
    {0, 1, 30},
    {1, 2, 30}, {2, 3, 30}, {3, 4, 30}, {1, 5, 30}, {5, 6, 30}, {6, 7, 30},
    {8, 9, 30}, {9, 10, 30}, {10, 11, 30}, {8, 12, 30}, {12, 13, 30}, {13, 14, 30},
    {1, 8, 40}, {2, 9, 40}, {5, 12, 40},
    {4, 18, 30}, {7, 17, 30}, {11, 16, 30}, {14, 15, 30}};

struct MaskLimb {          // one drawn limb that reaches this tile
  int ax, ay, bx, by;      // end points
  int dx, dy, L2;          // d = B - A, |d|^2
  int RR;                  // h*h + h: the round caps
  long long K;             // (2h+1)^2 * L2
};

struct MaskParams {
  const int32_t* peaks;    // [T][nj][2] (x, y), x < 0: joint off
  float* mask;             // [T][H][W], every element written
  int T, H, W, nj, tilesX;
  int vec;                 // 1: W % 4 == 0 and the base is 16-byte aligned, a lane's 4 pixels go out in one store
};

// grid (tilesX * tilesY, T), block 256.
__global__ __launch_bounds__(256) void k_human_mask(const MaskParams p) {
  __shared__ int2 s_pk[HMASK_MAXJ];
  __shared__ int4 s_disc[HMASK_MAXJ];          // (x, y, R*R + R, reaches the tile)
  __shared__ MaskLimb s_limb[HMASK_NLIMBS];
  __shared__ int s_hit[HMASK_NLIMBS];
  const int tid = threadIdx.x, t = blockIdx.y;
  const int ty = blockIdx.x / p.tilesX, tx = blockIdx.x - ty * p.tilesX;
  const int x0 = tx * HMASK_TW, y0 = ty * HMASK_TH;
  const int x1 = min(x0 + HMASK_TW, p.W) - 1, y1 = min(y0 + HMASK_TH, p.H) - 1;      // the tile's last column / row
  const int nlimbs = p.nj == 19 ? HMASK_NLIMBS : HMASK_NLIMBS - 4;
  const int32_t* pk = p.peaks + (size_t)t * p.nj * 2;

  // shape records of this tile, built once: a shape whose bounding box, grown by its half-width + 1, misses the tile is off
  int any = 0;
  if (tid < p.nj) {
    const int x = pk[2 * tid], y = pk[2 * tid + 1];
    s_pk[tid] = make_int2(x, y);
    const int R = tid == 0 ? 30 : 15;
    const int hit = x >= 0 && x + R + 1 >= x0 && x - R - 1 <= x1 && y + R + 1 >= y0 && y - R - 1 <= y1;
    s_disc[tid] = make_int4(x, y, R * R + R, hit);
    any |= hit;
  }
  __syncthreads();
  if (tid < nlimbs) {
    const int2 A = s_pk[kMaskLimbs[tid][0]], B = s_pk[kMaskLimbs[tid][1]];
    const int h = kMaskLimbs[tid][2] / 2;
    const int hit = A.x >= 0 && B.x >= 0 && max(A.x, B.x) + h + 1 >= x0 && min(A.x, B.x) - h - 1 <= x1 &&
                    max(A.y, B.y) + h + 1 >= y0 && min(A.y, B.y) - h - 1 <= y1;
    MaskLimb L;
    L.ax = A.x; L.ay = A.y; L.bx = B.x; L.by = B.y;
    L.dx = B.x - A.x; L.dy = B.y - A.y;
    L.L2 = L.dx * L.dx + L.dy * L.dy;
    L.RR = h * h + h;
    L.K = (long long)((2 * h + 1) * (2 * h + 1)) * L.L2;
    s_limb[tid] = L;
    s_hit[tid] = hit;
    any |= hit;
  }
  any = __syncthreads_or(any);

  const int py = y0 + (tid >> 4), px = x0 + (tid & 15) * 4;       // this lane's 4 pixels: (px..px+3, py)
  if (py >= p.H || px >= p.W) return;
  bool m[4] = {false, false, false, false};
  if (any) {                                                       // (uniform: a tile no shape reaches only writes zeros)
    for (int j = 0; j < p.nj; ++j) {
      const int4 D = s_disc[j];
      if (!D.w) continue;                                          // uniform across the workgroup
      const int vy = py - D.y, vy2 = vy * vy;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int vx = px + k - D.x;
        m[k] |= vx * vx + vy2 <= D.z;
      }
    }
    for (int e = 0; e < nlimbs; ++e) {
      if (!s_hit[e]) continue;                                     // uniform across the workgroup
      const MaskLimb L = s_limb[e];
      const int vy = py - L.ay, wy = py - L.by;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int vx = px + k - L.ax, wx = px + k - L.bx;
        bool in = vx * vx + vy * vy <= L.RR || wx * wx + wy * wy <= L.RR;          // the caps on A and B
        const int dot = vx * L.dx + vy * L.dy;
        const long long cross = (long long)(vx * L.dy - vy * L.dx);
        in |= L.L2 != 0 && dot >= 0 && dot <= L.L2 && 4 * cross * cross <= L.K;     // the slab between them
        m[k] |= in;
      }
    }
  }
  float* row = p.mask + ((size_t)t * p.H + py) * p.W;
  if (p.vec) {                                                     // W % 4 == 0: px + 3 < W, one 16-byte store
    *reinterpret_cast<float4*>(row + px) = make_float4(m[0] ? 1.f : 0.f, m[1] ? 1.f : 0.f, m[2] ? 1.f : 0.f, m[3] ? 1.f : 0.f);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (px + k < p.W) row[px + k] = m[k] ? 1.f : 0.f;
  }
}

}  // namespace rib
