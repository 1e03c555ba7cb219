// pixel_ops.hip.h — the two one-statement pixel arithmetics that kernels of BOTH objects of librib.so evaluate, each stated
// once: blend1 (k_conv_head's fused blend in kernels.hip.h / rib.o, k_blend in frame_kernels.hip.h / frame.o) and quantise_u8
// (k_quantise in frame_kernels.hip.h, k_panel in panel.hip.h, k_composite in composite.hip.h), and beside the latter the mask
// quantiser of the source-size composite, quantise_mask_u8.  No kernel is defined here: igemm.hip.h, frame_kernels.hip.h,
// panel.hip.h and composite.hip.h include it, and csrc/build.py hashes it into the stamp of every object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rib {

// fuse = img*m + dain*(1-m) (PGNR/models/evaluator.py:256-258) with torch's roundings: two products, one difference,
// one sum, nothing contracted into an fma - the stand-alone k_blend and the blend fused into the mask head agree bit
// for bit with each other and with the reference's expression
__device__ __forceinline__ float blend1(float img, float m, float dain) {
  return __fadd_rn(__fmul_rn(img, m), __fmul_rn(dain, __fsub_rn(1.f, m)));
}

// uint8 HWC = uint8(clip(x*0.5+0.5, 0, 1)*255)  (truncation; PGNR/utils/utils.py:129-142; the
// reference evaluates this in float64, so do we).  One statement of the arithmetic for every kernel that writes a frame's
// bytes (k_quantise in frame_kernels.hip.h, k_panel in panel.hip.h); tests/golden/quant_ref.npz pins it to the reference's bytes.
__device__ inline uint8_t quantise_u8(float x) {
  double v = (double)x * 0.5 + 0.5;
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
  return (uint8_t)(v * 255.0);
}

// uint8 = uint8(clip(m, 0, 1)*255) of a blend mask (composite.composite_host's M; k_composite in composite.hip.h): the same
// shape of arithmetic without the affine map, in double so that no fp32 product rounds up across an integer (a float32
// times 255 is exact in double).  -0.0 compares equal to 0 and quantises to 0.
__device__ inline uint8_t quantise_mask_u8(float m) {
  double v = (double)m;
  v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
  return (uint8_t)(v * 255.0);
}

}  // namespace rib
