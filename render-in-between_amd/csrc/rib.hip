// rib.hip — runtime and C ABI (include/rib.h) of the MI355X-native generator.
//
// Host-side responsibilities (all native C++; Python only moves pointers):
//   * the layer inventory of the generator derived from rib_config
//     (reference: PGNR/models/generator.py:43-178,315-358,423-491);
//   * checkpoint ingestion in the reference's state-dict vocabulary, eval-mode spectral-norm
//     fold (PGNR/models/layers/weight_norm.py:84-85 hook), filter re-layout, one device blob;
//   * a static launch plan per (B,H,W): workspace layout + the ordered kernel launches that
//     restate Generator.forward (PGNR/models/generator.py:181-234) and MaskGenerator.forward
//     (:493-510) - its data model is plan.h, its builder planner.h, both parts of this translation unit;
//   * the autoregressive segment driver (PGNR/models/evaluator.py:238-262).
//
// The folder driver's frame utilities (rib_blend ... rib_jpeg) are a second object, frame.hip; rib_host.h holds what the two share.
#include "kernels.hip.h"
#include "rib_host.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <variant>
#include <vector>


// ---- the k_igemm instantiations live in the igemm_shard_<s>.o objects (variants.def, build.py) ----
#include "variants.hip.h"
#define RIB_V(sec, ...) RIB_I_V(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VK(sec, ...) RIB_I_VK(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VT(sec, ...) RIB_I_VT(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VTK(sec, ...) RIB_I_VTK(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_V9(sec, ...) RIB_I_V9(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VU4(sec, ...) RIB_I_VU4(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VS(sec, ...) RIB_I_VS(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VSK(sec, ...) RIB_I_VSK(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VB(sec, ...) RIB_I_VB(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VBX(sec, ...) RIB_I_VBX(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_V1D(sec, ...) RIB_I_V1D(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VS1D(sec, ...) RIB_I_VS1D(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VD(sec, ...) RIB_I_VD(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VSD(sec, ...) RIB_I_VSD(RIB_F_EXTERN, __VA_ARGS__)
#define RIB_VD9(sec, ...) RIB_I_VD9(RIB_F_EXTERN, __VA_ARGS__)
#include "variants.def"
#undef RIB_V
#undef RIB_VK
#undef RIB_VT
#undef RIB_VTK
#undef RIB_V9
#undef RIB_VU4
#undef RIB_VS
#undef RIB_VSK
#undef RIB_VB
#undef RIB_VBX
#undef RIB_V1D
#undef RIB_VS1D
#undef RIB_VD
#undef RIB_VSD
#undef RIB_VD9

using namespace rib;

// Every kernel launch of this file goes through RIB_KLAUNCH.  Outside a kernel-time profiling pass it is hipLaunchKernelGGL; inside
// one (rib_profile_begin_kernels) the launch carries a start and a stop event that the runtime binds to the dispatch itself
// (hipExtLaunchKernelGGL): their difference is the kernel's own execution time from the queue's timestamps - what rocprofv3's
// kernel trace reports - with no event packet between two launches.
namespace { struct ProfPair { hipEvent_t start = nullptr, stop = nullptr; }; thread_local ProfPair g_prof_pair; }
#define RIB_KLAUNCH(KERNEL, grid, block, lds, st, ...)                                                                       \
  do {                                                                                                                       \
    if (g_prof_pair.start) hipExtLaunchKernelGGL(KERNEL, grid, block, lds, st, g_prof_pair.start, g_prof_pair.stop, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL, grid, block, lds, st, __VA_ARGS__);                                                      \
  } while (0)

#if !defined(RIB_BUILD_STAMP) || !defined(RIB_SHARD_STAMP) || !defined(RIB_SHARED_STAMP)
#error "compile through csrc/build.py (-DRIB_BUILD_STAMP / -DRIB_SHARD_STAMP / -DRIB_SHARED_STAMP: content hashes of the sources, see build.py)"
#endif
// the stamp strings of the RIB_NSECTIONS k_igemm shard objects (igemm_shard.hip), of frame.o (frame.hip) and this object's own
extern "C" {
#define RIB_X(s) extern const char rib_stamp_section_##s[];
RIB_FOR_SECTIONS(RIB_X)
#undef RIB_X
extern const char rib_stamp_frame[];             // "rib-stamp frame <hash>"
extern const char rib_frame_shared_stamp[];      // the hash of the shared headers (rib_host.h ...) frame.o was compiled against
}
extern "C" __attribute__((used, visibility("hidden"))) const char kLibStamp[] = "rib-stamp lib " RIB_BUILD_STAMP;

namespace {

thread_local std::string g_create_error;

// channel padding of an activation: 8, 16, or a multiple of 32 (so that every tensor admits the
// 16- or 32-channel K chunks of the fast kernel variants; the 22-channel label map becomes 32)
inline int pad8(int c) { return c <= 8 ? 8 : (c <= 16 ? 16 : (c + 31) / 32 * 32); }
// bf16 storage: 16-channel K steps (v_mfma_f32_32x32x16_bf16), so the smallest activation is 16 channels wide
inline int pad16(int c) { return c <= 16 ? 16 : (c + 31) / 32 * 32; }
// float -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does on the device)
inline uint16_t host_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
// float -> IEEE half, round to nearest even (what v_cvt_f16_f32 does on the device), subnormals and overflow to inf included
inline uint16_t host_f16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                      // NaN
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                     // >= 65520 rounds to inf
  if (a < 0x33000001u) return (uint16_t)sign;                                  // <= 2^-25 rounds to zero
  int e = (int)(a >> 23) - 127;
  uint32_t m = (a & 0x7fffffu) | 0x800000u;                                    // 24-bit significand
  int shift = e < -14 ? 13 + (-14 - e) : 13;                                   // bits dropped (subnormal: more)
  uint32_t half_m = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (half_m & 1u))) half_m += 1;
  uint32_t h16;
  if (e < -14) h16 = half_m;                                                   // subnormal (a carry into 0x400 is the smallest normal: correct)
  else h16 = ((uint32_t)(e + 15) << 10) + (half_m - 0x400u);                   // a mantissa carry bumps the exponent: correct
  return (uint16_t)(sign | h16);
}
inline int pad32(int c) { return (c + 31) / 32 * 32; }
inline int pick_bk(int cp) { return cp % 32 == 0 ? 32 : (cp % 16 == 0 ? 16 : 8); }

// ------------------------------------------------------------------------------------------
// layer inventory (mirrors render_in_between_amd/spec.py; pinned by the state-dict key test)
// ------------------------------------------------------------------------------------------
struct ConvDef {
  std::string name;
  int cin = 0, cout = 0, ks = 3, stride = 1;
  bool spectral = true;
  int spade_cond = 0;
  bool in_affine = false;
  bool used = true;
  // device blob offsets (floats), filled by finalize
  size_t w_off = 0, b_off = 0, g_off = 0, be_off = 0;
  size_t fb_off = 0;   // conv_block_1 of a learned-shortcut SPADE block: bias + shortcut bias (fused launch)
  // convolution of a nearest-x2-upsampled tensor (mask network, generator.py:480): the launch runs on the
  // four 2x2 phase filters [CoutPad][16 = phase*4 + a*2 + b][CinPad] at wp_off (sums of the taps at w_off)
  bool ups_in = false;
  size_t wp_off = 0;
  int cinp = 0, coutp = 0;
  // bf16 storage mode: bf16 copies of the filters (same [CoutPad][tap][CinPad] layout), offsets in floats of the blob
  size_t w16_off = 0, wp16_off = 0;
  // Winograd: the layer may run in the Winograd domain (wino_ok); the transformed filter sets U = G g G^T live OUTSIDE the
  // blob, made on the device from the folded filters when a plan first needs one (WinoSet, ensure_wino_set); zero_off: a
  // zero bias vector for the batched GEMM (the real bias is added by the output transform)
  bool wino_ok = false; size_t zero_off = 0;
  bool wino_s_ok = false;   // conv_block_1 of a learned-shortcut block: may run in the Winograd domain with the shortcut fused in (no blob space)
  size_t wl_off = 0; int lowc_ce = 0, lowc_ncol = 0;   // k_conv_lowc filter [9*CE/KG][KG][NCOL] (real-channel K order), CE / NCOL of its instantiation
};

struct TensorDef {
  std::string name;
  std::vector<int64_t> dims;
  bool used;
  std::vector<float> data;
  bool set = false;
};

struct SpadeGroup {   // one SPADE launch: 1 or 2 modulations sharing the normalised tensor
  std::string key;    // "<block>.0s" / "<block>.0" / "<block>.1"
  int C = 0, Cp = 0, cond = 0, nsets = 1;
  size_t w_off = 0, b_off = 0;
  size_t w16_off = 0; // bf16 copy of the gamma/beta filters (bf16 storage mode)
  int npad = 0;       // virtual columns (multiple of 64)
  // 16 modulated channels in all (C = 16, one set): a second copy in [gamma(16) | beta(16)] order, one 32-column
  // fragment instead of two half-empty ones (fp32 SPADE variants with NF = 1)
  size_t w1_off = 0, b1_off = 0;
  // condition level (index of the ref_embedding map this SPADE reads) and first column of this group inside the level's
  // concatenated gamma/beta filter matrix [sum of npad][cond] (the groups of a level are laid out back to back in the blob,
  // in execution order, so that ONE 1x1 GEMM on the level's map can produce the gamma/beta of all of them: cond_level_gemm)
  int level = 0, col0 = 0;
};

struct Cfg {
  rib_config c;
  int nf(int i) const { return std::min(c.max_num_filters, c.num_filters << i); }
  int mask_nf(int i) const { return std::min(c.mask_max_filters, c.mask_filters << i); }
  int emb_ch(int i) const { return std::min(c.emb_max_filters, c.emb_filters << i); }
  int cond_ch(int i) const { return std::min(c.max_num_filters, c.emb_filters << std::min(i, c.emb_down)); }
  int num_res_blocks() const { return (int)std::ceil((c.num_layers - c.num_down_img) / 2.0) * 2; }
};

void add_embedder(std::vector<ConvDef>& L, const Cfg& g, const std::string& prefix, int cin, bool used) {
  ConvDef c; c.name = prefix + ".conv_first"; c.cin = cin; c.cout = g.emb_ch(0); c.used = used; L.push_back(c);
  for (int i = 0; i < g.c.emb_down; ++i) {
    ConvDef d; d.name = prefix + ".down_" + std::to_string(i); d.cin = g.emb_ch(i); d.cout = g.emb_ch(i + 1);
    d.stride = 2; d.used = used; L.push_back(d);
  }
}
void add_spade_block(std::vector<ConvDef>& L, const std::string& name, int cin, int cout, int cond) {
  const int hidden = std::min(cin, cout);
  ConvDef a; a.name = name + ".conv_block_0"; a.cin = cin; a.cout = hidden; a.spade_cond = cond; L.push_back(a);
  ConvDef b; b.name = name + ".conv_block_1"; b.cin = hidden; b.cout = cout; b.spade_cond = cond; L.push_back(b);
  if (cin != cout) {
    ConvDef s; s.name = name + ".conv_block_s"; s.cin = cin; s.cout = cout; s.ks = 1; s.spade_cond = cond; L.push_back(s);
  }
}
void add_mask_block(std::vector<ConvDef>& L, const std::string& name, int cin, int cout) {
  const int hidden = std::min(cin, cout);
  ConvDef a; a.name = name + ".conv_block_0"; a.cin = cin; a.cout = hidden; a.in_affine = true; L.push_back(a);
  ConvDef b; b.name = name + ".conv_block_1"; b.cin = hidden; b.cout = cout; b.in_affine = true; L.push_back(b);
  if (cin != cout) {
    ConvDef s; s.name = name + ".conv_block_s"; s.cin = cin; s.cout = cout; s.ks = 1; s.in_affine = true; L.push_back(s);
  }
}

std::vector<ConvDef> build_inventory(const Cfg& g) {
  std::vector<ConvDef> L;
  const rib_config& c = g.c;
  add_embedder(L, g, "ref_embedding", c.image_nc * 2, true);
  add_embedder(L, g, "label_embedding", c.label_nc, false);
  for (int i = c.num_down_img; i >= 0; --i) add_spade_block(L, "up_" + std::to_string(i), g.nf(i + 1), g.nf(i), g.cond_ch(i));
  { ConvDef d; d.name = "conv_img"; d.cin = c.num_filters; d.cout = c.image_nc; d.spectral = false; L.push_back(d); }
  { ConvDef d; d.name = "conv_mask"; d.cin = c.num_filters; d.cout = 1; d.spectral = false; d.used = false; L.push_back(d); }
  { ConvDef d; d.name = "down_first"; d.cin = c.label_nc; d.cout = c.num_filters; d.spectral = false; L.push_back(d); }
  for (int i = 0; i <= c.num_down_img; ++i) add_spade_block(L, "down_" + std::to_string(i), g.nf(i), g.nf(i + 1), g.cond_ch(i));
  const int res_ch = g.nf(c.num_down_img + 1);
  for (int i = 0; i < g.num_res_blocks(); ++i) add_spade_block(L, "res_" + std::to_string(i), res_ch, res_ch, g.cond_ch(c.num_down_img + 1));
  const std::string m = "flow_network_temp";
  const char* branches[2] = {"down_lbl", "down_img"};
  const int bcin[2] = {c.label_nc, c.image_nc * 3};
  for (int b = 0; b < 2; ++b) {
    ConvDef d; d.name = m + "." + branches[b] + ".0"; d.cin = bcin[b]; d.cout = c.mask_filters; d.in_affine = true; L.push_back(d);
    for (int i = 0; i < c.mask_down; ++i) {
      ConvDef e; e.name = m + "." + branches[b] + "." + std::to_string(i + 1); e.cin = g.mask_nf(i); e.cout = g.mask_nf(i + 1);
      e.stride = 2; e.in_affine = true; L.push_back(e);
    }
  }
  const int ch = g.mask_nf(c.mask_down);
  for (int i = 0; i < c.mask_res_blocks; ++i) add_mask_block(L, m + ".res_flow." + std::to_string(i), i == 0 ? ch * 2 : ch, ch);
  for (int j = 0; j < c.mask_down; ++j) {
    const int i = c.mask_down - 1 - j;
    ConvDef d; d.name = m + ".up_flow." + std::to_string(2 * j + 1); d.cin = g.mask_nf(i + 1); d.cout = g.mask_nf(i); d.in_affine = true; d.ups_in = true; L.push_back(d);
  }
  { ConvDef d; d.name = m + ".conv_mask.0"; d.cin = c.mask_filters; d.cout = 1; d.spectral = false; L.push_back(d); }
  return L;
}

// ------------------------------------------------------------------------------------------
// kernel variant table
// ------------------------------------------------------------------------------------------
typedef void (*IgemmFn)(const IgemmParams);
struct Variant {
  int FRW, WM, WN, MF, NF, BK, STRIDE, KS; bool UPS, SPADE;
  IgemmFn fn;          // generic instantiation (fused-shortcut loop and input prologue compiled in)
  int BF16 = 0;        // precision of this instantiation: PREC_F32 / PREC_BF16 / PREC_F16 (16-bit storage)
  IgemmFn fn_pro = nullptr;    // without the fused-shortcut loop
  IgemmFn fn_lean = nullptr;   // without the fused-shortcut loop and without the prologue
  int KW = 1;                  // in-workgroup split-K: KW groups of 4 waves (256*KW threads) per tile
  int TB = 1;                  // filter slices staged per barrier: 1 tap, or 3 = one row of a 3x3 filter
  // FRW == 0: not a k_igemm instantiation but a tile of k_gemm_dma (plain GEMM, operands staged by LDS-DMA): (32 WM) x (32 NF WN),
  // fp32 only; serves the batched Winograd-domain GEMMs and the condition-level gamma/beta GEMM
  int DMAK = 0;                // k_igemm instantiations whose operand tiles are staged by LDS-DMA (filters always, the input tile in
                               // the lean one); no fused-shortcut instantiation; reported as TB = 100 in the exported geometry
  typedef void (*GemmDmaFn)(const GemmDmaParams);
  GemmDmaFn gfn = nullptr;
  GemmDmaFn gfn_x3 = nullptr;  // the same tile with split-bf16 products (rib_set_products(RIB_PRODUCTS_BF16X3); fp32 storage only)
  bool dma() const { return FRW == 0; }
  int BM() const { return 32 * WM; }
  int TH() const { return (32 / FRW) * MF * WM; }
  int TW() const { return FRW; }
  int BN() const { return NF == 0 ? 16 * WN : 32 * NF * WN; }   // NF == 0: 16-column MFMA path
  int lds_bytes() const {
    if (dma()) return 2 * (BM() + BN()) * 32 * 4;
    if (DMAK) {      // IgemmGeom with DMA: unpadded rows, whole DMA instructions, two input-tile buffers (lean) - the larger of lean / prologue
      const int ih_ = (TH() - 1) * STRIDE + KS, iw_ = (TW() - 1) * STRIDE + KS;
      const int iwp_ = (STRIDE == 2 && FRW == 8) ? ((iw_ + 3) / 8 * 8 + 4) : iw_;
      const int sl = BK / 4;
      const int sb = (BN() * sl + 255) / 256 * 256 * 4;
      const int lean = 2 * ((ih_ * iwp_ * sl + 255) / 256 * 256 * 4) + 2 * TB * sb, pro = ih_ * iwp_ * (BK + 4) + 2 * sb;
      return (TB == 9 || lean > pro ? lean : pro) * 4;
    }
    const int ih = UPS ? TH() + 2 : (TH() - 1) * STRIDE + KS, iw = UPS ? TW() + 2 : (TW() - 1) * STRIDE + KS;
    const int iwp = (STRIDE == 2 && FRW == 8) ? ((iw + 3) / 8 * 8 + 4) : iw;   // IgemmGeom::IWP
    const int ck = (BF16 != PREC_F32 ? BK / 2 : BK) + 4;   // IgemmGeom::CK
    const bool db1 = KS == 1 && TB == 2;                                                        // 1x1, everything double-buffered
    const int main_loop = (((TB == 9 || db1) ? 2 : 1) * ih * iwp * ck + 2 * (db1 ? 1 : TB) * BN() * ck) * 4;   // IgemmGeom::NA, TBB
    const int kw_reduce = KW > 1 ? (NF == 0 ? 1 : NF) * MF * 16 * 256 * 4 : 0;
    return main_loop > kw_reduce ? main_loop : kw_reduce;
  }
};
// RIB_V: convolution geometries, three instantiations (generic / no shortcut loop / lean); the
// shortcut loop only exists for 3x3 stride-1 gathers, elsewhere "generic" already is "pro".
// RIB_VS: SPADE geometries (one instantiation).  RIB_VB: bf16 twins (generic only).
#define RIB_V(sec, FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP)                                                         \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP,                                                             \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, false, (KS == 3 && S == 1 && !UPS), true>, false,   \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, false, false, true>,                               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, false, false, false>},
// RIB_VK: in-workgroup split-K twin of a convolution geometry (fp32, 32-column path)
#define RIB_VK(sec, FRW, WM, WN, MF, NF, BK, S, KS, UPS, KW)                                                                  \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, false,                                                                    \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, false, false, (KS == 3 && S == 1 && !UPS), true, KW>, false,      \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, false, false, false, true, KW>,                                  \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, false, false, false, false, KW>, KW},
// RIB_VT: three-taps-per-barrier twin of a 3x3 convolution geometry
#define RIB_VT(sec, FRW, WM, WN, MF, NF, BK, S, UPS)                                                                         \
  Variant{FRW, WM, WN, MF, NF, BK, S, 3, UPS, false,                                                                    \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, UPS, false, false, (S == 1 && !UPS), true, 1, 3>, false,               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, UPS, false, false, false, true, 1, 3>,                                \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, UPS, false, false, false, false, 1, 3>, 1, 3},
// RIB_VTK: three taps per barrier AND KW wave groups per tile (8 / 16 waves share the 3-slice filter buffers)
#define RIB_VTK(sec, FRW, WM, WN, MF, NF, BK, S, KW)                                                                         \
  Variant{FRW, WM, WN, MF, NF, BK, S, 3, false, false,                                                                  \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, false, (S == 1), true, KW, 3>, false,                    \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, false, false, true, KW, 3>,                             \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, false, false, false, KW, 3>, KW, 3},
// RIB_V9: all nine filter slices of a chunk per barrier pair (TB = 9), optionally with KW wave groups
#define RIB_V9(sec, FRW, WM, WN, MF, NF, BK, S, KW)                                                                          \
  Variant{FRW, WM, WN, MF, NF, BK, S, 3, false, false,                                                                  \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, false, (S == 1), true, KW, 9>, false,                    \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, false, false, true, KW, 9>,                             \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, false, false, false, KW, 9>, KW, 9},
// RIB_VU4: phase-decomposed upsample convolution with the four taps of a phase per barrier (TB = 4)
#define RIB_VU4(sec, FRW, WM, WN, MF, NF, BK)                                                                                \
  Variant{FRW, WM, WN, MF, NF, BK, 1, 3, true, false,                                                                   \
          &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 3, true, false, false, false, true, 1, 4>, false,                         \
          &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 3, true, false, false, false, true, 1, 4>,                               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 3, true, false, false, false, false, 1, 4>, 1, 4},
#define RIB_VS(sec, FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP) \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, false>, false},
// RIB_VSK: in-workgroup split-K twin of a SPADE geometry: the fused kernel on the small deep maps with 8 / 16 waves
// per tile instead of the unfused pair (split-K GEMM into slabs + k_spade_modulate)
#define RIB_VSK(sec, FRW, WM, WN, MF, NF, BK, KW) \
  Variant{FRW, WM, WN, MF, NF, BK, 1, 1, false, true, &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 1, false, true, false, true, true, KW>, false, nullptr, nullptr, KW},
// (every 16-bit geometry exists twice: bf16 and half elements, PREC_BF16 / PREC_F16)
#define RIB_VB(sec, FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP) \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, 1>, 1}, \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, 2>, 2},
// 1x1, everything double-buffered (TB = 2): convolution (pro / lean) and SPADE
#define RIB_V1D(sec, FRW, WM, WN, MF, NF, BK, KW)                                                                    \
  Variant{FRW, WM, WN, MF, NF, BK, 1, 1, false, false,                                                               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 1, false, false, 0, false, true, KW, 2>, 0,                            \
          &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 1, false, false, 0, false, true, KW, 2>,                               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 1, false, false, 0, false, false, KW, 2>, KW, 2},
#define RIB_VS1D(sec, FRW, WM, WN, MF, NF, BK, KW) \
  Variant{FRW, WM, WN, MF, NF, BK, 1, 1, false, true, &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 1, false, true, 0, true, true, KW, 2>, 0, nullptr, nullptr, KW, 2},
#define RIB_VBX(sec, FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, KW, TB)                                                            \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP,                                                                               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, 1, (KS == 3 && S == 1 && !UPS && !SP), true, KW, TB>, 1, nullptr, nullptr, KW, TB}, \
  Variant{FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP,                                                                               \
          &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, UPS, SP, 2, (KS == 3 && S == 1 && !UPS && !SP), true, KW, TB>, 2, nullptr, nullptr, KW, TB},

// RIB_VD / RIB_VSD: LDS-DMA-staged twins (variants.def)
#define RIB_VD(sec, FRW, WM, WN, MF, NF, BK, S, KS) \
  dmak_variant(Variant{FRW, WM, WN, MF, NF, BK, S, KS, false, false, nullptr, 0,                                          \
                       &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, false, false, 0, false, true, 1, 1, 1>,                   \
                       &k_igemm<FRW, WM, WN, MF, NF, BK, S, KS, false, false, 0, false, false, 1, 1, 3>}),
#define RIB_VSD(sec, FRW, WM, WN, MF, NF, BK) \
  dmak_variant(Variant{FRW, WM, WN, MF, NF, BK, 1, 1, false, true, &k_igemm<FRW, WM, WN, MF, NF, BK, 1, 1, false, true, 0, false, false, 1, 1, 3>, 0}),

#define RIB_VD9(sec, FRW, WM, WN, MF, NF, BK, S) \
  dmak_variant(Variant{FRW, WM, WN, MF, NF, BK, S, 3, false, false, nullptr, 0, nullptr,                                   \
                       &k_igemm<FRW, WM, WN, MF, NF, BK, S, 3, false, false, 0, false, false, 1, 9, 3>, 1, 9}),

// the leanest instantiation that covers a launch
inline IgemmFn pick_igemm_fn(const Variant* v, const IgemmParams& p) {
  if (p.x2 != nullptr || (v->fn && !v->fn_pro)) return v->fn;
  if (p.pro_scale == nullptr && !p.pro_lrelu && v->fn_lean) return v->fn_lean;
  return v->fn_pro ? v->fn_pro : v->fn;
}

inline Variant dmak_variant(Variant v) { v.DMAK = 1; return v; }
inline Variant dma_variant(int WM, int WN, int NF, Variant::GemmDmaFn fn, int prec = PREC_F32, Variant::GemmDmaFn fn_x3 = nullptr) {
  Variant v{0, WM, WN, 1, NF, prec == PREC_F32 ? 32 : 64, 1, 1, false, false, nullptr};      // BK: elements of a 128-byte row chunk
  v.gfn = fn;
  v.gfn_x3 = fn_x3;
  v.BF16 = prec;
  return v;
}
// split-bf16 twin of an fp32 tile: the hh products in their own accumulator where the registers allow it (NF <= 2)
#define RIB_DMA_X3(WM, WN, NF) PREC_F32, &k_gemm_dma<WM, WN, NF, ST_F32, (NF <= 2 ? 2 : 1)>
const Variant kVariants[] = {
#include "variants.def"
    // k_gemm_dma tiles (instantiated in this translation unit): 128x64, 64x64, 64x128, 128x128, 128x32
    dma_variant(4, 1, 2, &k_gemm_dma<4, 1, 2>, RIB_DMA_X3(4, 1, 2)), dma_variant(2, 2, 1, &k_gemm_dma<2, 2, 1>, RIB_DMA_X3(2, 2, 1)),
    dma_variant(2, 2, 2, &k_gemm_dma<2, 2, 2>, RIB_DMA_X3(2, 2, 2)), dma_variant(4, 1, 4, &k_gemm_dma<4, 1, 4>, RIB_DMA_X3(4, 1, 4)),
    dma_variant(4, 1, 1, &k_gemm_dma<4, 1, 1>, RIB_DMA_X3(4, 1, 1)),
    // ... and their 16-bit storage twins (the condition-level GEMMs of the bf16 / half modes)
    dma_variant(4, 1, 2, &k_gemm_dma<4, 1, 2, ST_BF16>, PREC_BF16), dma_variant(2, 2, 1, &k_gemm_dma<2, 2, 1, ST_BF16>, PREC_BF16),
    dma_variant(2, 2, 2, &k_gemm_dma<2, 2, 2, ST_BF16>, PREC_BF16), dma_variant(4, 1, 4, &k_gemm_dma<4, 1, 4, ST_BF16>, PREC_BF16),
    dma_variant(4, 1, 2, &k_gemm_dma<4, 1, 2, ST_F16>, PREC_F16), dma_variant(2, 2, 1, &k_gemm_dma<2, 2, 1, ST_F16>, PREC_F16),
    dma_variant(2, 2, 2, &k_gemm_dma<2, 2, 2, ST_F16>, PREC_F16), dma_variant(4, 1, 4, &k_gemm_dma<4, 1, 4, ST_F16>, PREC_F16),
};
const int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

// Choose (variant, split-K factor) with a small analytic cost model, in shader cycles:
//   per wave and tap   (BK/8)*MF*NF*4 MFMAs of 64 cycles + a fixed barrier/LDS overhead
//   latency bound      rounds of resident workgroups x the dependent chain of one workgroup
//   matrix-core bound  each CU runs the MFMAs of its workgroups serially on its 4 SIMDs
// A split-K launch pays a second (slab-summing) kernel.
struct Choice { const Variant* v = nullptr; int ksplit = 1; double cycles = 0; };

Choice choose_variant_dt(int bf16, int stride, int ks, bool ups, bool spade, int ncols, int B, int Hout, int Wout,
                         int Cin, bool allow_split, int Cin2, bool allow_n16);

Choice choose_variant(int bf16, int stride, int ks, bool ups, bool spade, int ncols, int B, int Hout, int Wout,
                      int Cin, bool allow_split, int Cin2 = 0, bool allow_n16 = false) {
  // a bf16 handle stores bf16 activations: only the bf16 kernels can read them
  return choose_variant_dt(bf16, stride, ks, ups, spade, ncols, B, Hout, Wout, Cin, allow_split, Cin2, allow_n16 && bf16 == PREC_F32);
}

Choice choose_variant_dt(int bf16, int stride, int ks, bool ups, bool spade, int ncols, int B, int Hout, int Wout,
                         int Cin, bool allow_split, int Cin2, bool allow_n16) {
  Choice best;
  best.cycles = 1e300;
  static const int kSplits[] = {1, 2, 3, 4, 6, 8, 12, 16};
  for (int i = 0; i < kNumVariants; ++i) {
    const Variant& v = kVariants[i];
    if (v.dma() || v.DMAK) continue;        // (k_gemm_dma tiles: pick_gemm_dma; DMA-staged k_igemm twins: tuned choices only)
    if (v.STRIDE != stride || v.KS != ks || v.UPS != ups || v.SPADE != spade || Cin % v.BK != 0 || Cin2 % v.BK != 0) continue;
    if (v.NF == 0 && !allow_n16) continue;
    if (v.SPADE && v.NF == 1) continue;      // 16-channel SPADE layout: chosen explicitly (Builder::spade)
    if (v.BF16 != bf16) continue;   // (bf16 carries the handle's precision mode)
    const int BK = v.BK;
    // in-workgroup split-K only where the tile grid alone cannot fill the chip
    if ((v.KW > 1 || v.TB > 1) && (long)((Hout + v.TH() - 1) / v.TH()) * ((Wout + v.TW() - 1) / v.TW()) * ((ncols + v.BN() - 1) / v.BN()) * B >= 512) continue;
    const int nchunks = Cin / BK;
    // phase-decomposed upsample conv: tiles of SOURCE pixels, 16 (phase, tap) steps per chunk
    const int Ht = ups ? Hout / 2 : Hout, Wt = ups ? Wout / 2 : Wout;
    const long tiles = (long)((Ht + v.TH() - 1) / v.TH()) * ((Wt + v.TW() - 1) / v.TW());
    const long ntiles = v.NF == 0 ? 1 : (ncols + v.BN() - 1) / v.BN();
    const int occ = std::max(1, std::min(v.MF * v.NF * (ups ? 4 : 1) >= 4 ? 4 : 6, 160 * 1024 / v.lds_bytes()));
    for (int S : kSplits) {
      if (S > nchunks || (S > 1 && (!allow_split || v.NF == 0))) break;
      const long wgs = tiles * ntiles * B * S;
      const int chunks = (nchunks + S - 1) / S;
      const int taps = ups ? 16 : ks * ks;
      const double mfma_tap = v.NF == 0 ? (BK / 16) * v.MF * 8 * 32.0
                                        : (v.BF16 != PREC_F32 ? (BK / 16) * v.MF * v.NF * 32.0 : (BK / 8) * v.MF * v.NF * 4 * 64.0);
      // per tap: barrier + LDS write/read latency; per chunk: halo-tile commit; per workgroup:
      // first global loads (HBM latency) + epilogue.  Overheads of one workgroup hide behind the
      // matrix work of the other `occ` resident ones (measured: occupancy is the dominant lever).
      // in-workgroup split-K: KW wave groups interleave on the same SIMDs, which hides 1/KW more of the
      // overheads; the accumulator hand-over costs two barriers and 16 KB of LDS traffic per extra group
      const double ovh_wg = (chunks * (std::max(1, taps / v.TB) * 350.0 + (ks == 1 && v.TB == 2 ? 300.0 : 600.0)) + 7000.0) / v.KW + (v.KW - 1) * 1500.0;
      const double mfma_wg = (double)chunks * taps * mfma_tap;
      const double t_lat = std::ceil((double)wgs / (256.0 * occ)) * (mfma_wg + ovh_wg);
      const double t_cu = std::ceil((double)wgs / 256.0) * (mfma_wg + ovh_wg / occ);
      double t = std::max(t_lat, t_cu);
      if (S > 1) t += 6000.0 + (double)(S + 1) * B * Hout * Wout * pad32(ncols) * 4.0 / 1667.0;
      if (t < best.cycles) { best.cycles = t; best.v = &v; best.ksplit = S; }
    }
  }
  return best;
}

// default k_gemm_dma tile of a Z x [M x N x K] problem: the largest tile that still gives two workgroups per CU, else the
// tile with the most workgroups (RIB_NO_DMA=1: none - the callers fall back to k_igemm's 1x1 variants)
const Variant* pick_gemm_dma(int prec, long Z, int M, int N, int K) {
  static const bool off = getenv("RIB_NO_DMA") != nullptr;
  if (off || K % (prec == PREC_F32 ? 32 : 64) != 0) return nullptr;
  const Variant* best = nullptr; long best_area = 0, best_wgs = 0;
  for (int i = 0; i < kNumVariants; ++i) {
    const Variant& v = kVariants[i];
    if (!v.dma() || v.BF16 != prec) continue;
    const long wgs = Z * ((M + v.BM() - 1) / v.BM()) * ((N + v.BN() - 1) / v.BN());
    const long area = (long)v.BM() * v.BN();
    const bool full = wgs >= 512, bfull = best_wgs >= 512;
    if (!best || (full && (!bfull || area > best_area)) || (!full && !bfull && wgs > best_wgs)) { best = &v; best_area = area; best_wgs = wgs; }
  }
  return best;
}

}  // namespace

#include "plan.h"      // PRef, Op, OpOf, Act, Norm, LazySrc, Plan: the plan's data model

struct rib_handle : rib::FrameState {     // device, err, label_nc and the frame utilities' own state: rib_host.h
  Cfg g;
  std::vector<ConvDef> convs;
  std::map<std::string, int> conv_index;
  std::vector<TensorDef> tensors;
  std::map<std::string, int> tensor_index;
  std::vector<SpadeGroup> spades;
  std::map<std::string, int> spade_index;
  std::map<int, std::vector<int>> level_groups;   // condition level -> its SPADE groups (indices into spades), execution order
  float* d_blob = nullptr;
  size_t d_blob_floats = 0;      // allocated size (the bf16 storage mode carries bf16 filter copies: a larger blob)
  std::vector<float> host_blob;   // host-only handles (device < 0) keep the folded blob here
  size_t blob_floats = 0;
  size_t zero_off = 0;            // 64 floats of zeros in the blob: the source of zero-padding pixels for DMA-staged input tiles
  uint64_t layout_hash = 0;       // of the blob's offsets (assign_weight_layout); part of the blob header
  // Winograd-domain filter sets U = G g G^T, [positions][CoutPad][CinPad] fp32 each, made on the device from the folded
  // filters of the blob when a plan first asks for one (round 3: they were 391 of the blob's 514 MB, both sets of every layer,
  // folded on the host, uploaded and broadcast; a 512x512 frame uses 17 of the 34)
  // aux >= 0: the set also carries the 1x1 shortcut convolution `aux` as extra K columns (rows of cinp + its cinp floats)
  struct WinoSet { int conv = 0, wm = 0; float* d = nullptr; size_t floats = 0; int aux = -1; };
  std::vector<WinoSet> wino_sets;
  std::map<std::array<int, 3>, int> wino_index;      // (conv, wm, aux)
  bool weights_ready = false;
  int prec_mode = PREC_F32;    // rib_set_compute_dtype: PREC_BF16 / PREC_F16 = 16-bit storage + 16-bit matrix-core operands
  int prec() const { return prec_mode; }
  int products = 0;            // rib_set_products: RIB_PRODUCTS_BF16X3 = the k_gemm_dma launches of the fp32 mode run their split-bf16 twins
  bool mc16() const { return prec_mode != PREC_F32; }                    // the matrix-core kernels read 16-bit filter copies, 16-channel steps
  int padc(int c) const { return mc16() ? pad16(c) : pad8(c); }          // channel padding of an activation
  int esz() const { return mc16() ? 2 : 4; }                       // bytes per stored activation element
  // rib_set_wino_in_staging: the Winograd input transforms stage each input patch in LDS once (k_wino_in_staged); off = every
  // unit fetches its own rows (k_wino_in / k_wino4_in).  Same V and the same launch list either way; RIB_WINO_IN_UNSTAGED=1
  // in the environment of rib_create starts a handle with it off
  bool wino_in_staging = true;
  bool keep_taps = false;      // rib_set_debug_taps: intermediate activations stay intact until the end of a forward
  // rib_set_plan_batch: > 0 = every launch plan, whatever its batch, follows the kernel choices (tuned table / cost model, split-K,
  // Winograd tile, fused or level-wise SPADE) of THIS batch size, so that a sample's arithmetic does not depend on how many other
  // samples ran beside it (the folder driver: frames independent of segment grouping and of the world size); 0 = each batch its own
  int plan_batch = 0;
  std::map<std::array<int, 5>, std::unique_ptr<Plan>> plans;      // key {flags, tuneB, B, H, W}: see get_plan
  // tuned (variant, split-K) per "B,H,W|op name"; consulted before the analytic cost model
  std::map<std::string, std::pair<int, int>> choices;
  // profiling
  // rib_chain graph replay (rib_set_graph_replay / RIB_GRAPH=1): instantiated graphs of whole segments, keyed by everything a
  // launch parameter depends on - the shape and every pointer of the call; least recently used first out
  struct ChainGraph { std::array<uintptr_t, 12> key; hipGraphExec_t exec; uint64_t used; hipStream_t stream; };   // stream: of its last launch
  std::vector<ChainGraph> chain_graphs;
  bool graph_replay = false;
  uint64_t graph_clock = 0, graph_captures = 0, graph_replays = 0;
  bool profiling = false;
  bool prof_kernels = false;   // rib_profile_begin_kernels: (start, stop) pairs bound to the dispatches instead of interval events
  std::vector<std::pair<int, hipEvent_t>> prof_events;   // (class of the launch behind the event, -1: end of a plan run)
  struct KernelEv { int kclass; hipEvent_t start, stop; };
  std::vector<KernelEv> prof_kernel_events;
  int64_t prof_launches[RIB_KC_COUNT] = {0};
  double prof_ms[RIB_KC_COUNT] = {0};
};

__attribute__((visibility("hidden"))) rib::FrameState* rib::frame_state(rib_handle* h) { return h; }

namespace {

// instantiated chain graphs hold the plans' kernel parameters: whatever rebuilds plans or moves the blob drops them
// an instantiated graph may still be queued or running on the stream of its last launch (the launch only enqueues): that stream
// is drained before the executable goes away (evictions and plan changes are rare; a replay never comes here)
void destroy_chain_graph(rib_handle::ChainGraph& g) {
  // The graph may have been replayed on several streams (the key does not hold the stream) and a stream of an earlier replay may
  // be gone by now: wait for the whole device instead of for the last stream alone.  Evictions and plan changes are rare; a
  // replay never comes here.  (rib_set_choice / rib_set_plan_batch / rib_set_products therefore BLOCK the host when the handle
  // holds captured segments: include/rib.h says so.)
  (void)hipDeviceSynchronize();
  (void)hipGraphExecDestroy(g.exec);
}
void drop_chain_graphs(rib_handle* h) {
  if (h->chain_graphs.empty()) return;
  if (h->device >= 0) (void)hipSetDevice(h->device);      // (the device-wide wait below must be this handle's device)
  for (auto& g : h->chain_graphs) destroy_chain_graph(g);
  h->chain_graphs.clear();
}

const ConvDef& conv_of(const rib_handle* h, const std::string& name) {
  return h->convs[h->conv_index.at(name)];
}

// ------------------------------------------------------------------------------------------
// Winograd-domain filter sets, made on the device from the folded 3x3 filters
// ------------------------------------------------------------------------------------------
// U[xi = T r + q][o][i] = (G g G^T)[r][q], T = m + 2, g[dy][dx] = w[o][dy*3+dx][i] (the blob's [CoutPad][9][CinPad] layout; padded
// rows / columns are zeros and stay zeros).  fp64 with the roundings of the plain expression (no contraction), stored fp32.
// F(2x2): G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1].  F(4x4): Cook-Toom with the points {0, +-3/4, +-3/2, inf}
// (kernels.hip.h, k_wino4_in): G[j] = (1, a_j, a_j^2) / prod_{k != j} (a_j - a_k), last row (0, 0, 1).
// ldu: floats of a row of U (cinp, or cinp + the channels of a fused 1x1 shortcut: k_wino_filters_1x1 fills that tail)
__global__ __launch_bounds__(256) void k_wino_filters(const float* w, float* u, int coutp, int cinp, int wm, int ldu) {
#pragma clang fp contract(off)
  const double G2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  const double G4[6][3] = {{64.0 / 81, 0, 0},
                           {-128.0 / 243, -32.0 / 81, -8.0 / 27}, {-128.0 / 243, 32.0 / 81, -8.0 / 27},
                           {32.0 / 243, 16.0 / 81, 8.0 / 27},     {32.0 / 243, -16.0 / 81, 8.0 / 27},
                           {0, 0, 1}};
  const int T = wm + 2;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)coutp * cinp) return;
  const int o = (int)(idx / cinp), i = (int)(idx % cinp);
  double g[3][3], t[6][3];
  for (int k = 0; k < 9; ++k) g[k / 3][k % 3] = (double)w[((size_t)o * 9 + k) * cinp + i];
  for (int r = 0; r < T; ++r)
    for (int dx = 0; dx < 3; ++dx) {
      const double* Gr = wm == 2 ? G2[r] : G4[r];
      t[r][dx] = Gr[0] * g[0][dx] + Gr[1] * g[1][dx] + Gr[2] * g[2][dx];
    }
  for (int r = 0; r < T; ++r)
    for (int q = 0; q < T; ++q) {
      const double* Gq = wm == 2 ? G2[q] : G4[q];
      u[((size_t)(r * T + q) * coutp + o) * ldu + i] = (float)(t[r][0] * Gq[0] + t[r][1] * Gq[1] + t[r][2] * Gq[2]);
    }
}
// The learned 1x1 shortcut of a res block as extra K columns of conv_block_1's set: a 1x1 filter is the 3x3 filter with only
// its centre tap, so U_s[r][q] = (G[r][1] w) G[q][1] - zero wherever r or q is a first / last row of G (12 of 16 / 20 of 36
// positions: the GEMM never reads those, GemmDmaParams::kmask).  w: [coutp][cin2] (the blob's 1x1 layout), columns col0.. of U.
__global__ __launch_bounds__(256) void k_wino_filters_1x1(const float* w, float* u, int coutp, int cin2, int wm, int ldu, int col0) {
#pragma clang fp contract(off)
  const double G2c[4] = {0, 0.5, -0.5, 0};
  const double G4c[6] = {0, -32.0 / 81, 32.0 / 81, 16.0 / 81, -16.0 / 81, 0};
  const int T = wm + 2;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)coutp * cin2) return;
  const int o = (int)(idx / cin2), i = (int)(idx % cin2);
  const double g = (double)w[(size_t)o * cin2 + i];
  for (int r = 0; r < T; ++r)
    for (int q = 0; q < T; ++q) {
      const double gr = wm == 2 ? G2c[r] : G4c[r], gq = wm == 2 ? G2c[q] : G4c[q];
      u[((size_t)(r * T + q) * coutp + o) * ldu + col0 + i] = (float)((gr * g) * gq);
    }
}

// (re)compute set `si` from the blob on `st`; the caller orders it against whatever reads the set
int fill_wino_set(rib_handle* h, int si, hipStream_t st) {
  rib_handle::WinoSet& ws = h->wino_sets[si];
  const ConvDef& c = h->convs[ws.conv];
  if (!ws.d || !h->d_blob) return RIB_OK;
  const size_t n = (size_t)c.coutp * c.cinp;
  const int k2 = ws.aux >= 0 ? h->convs[ws.aux].cinp : 0;
  RIB_KLAUNCH(k_wino_filters, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->d_blob + c.w_off, ws.d, c.coutp, c.cinp, ws.wm, c.cinp + k2);
  HIP_TRY(h, hipGetLastError());
  if (k2) {
    const size_t n2 = (size_t)c.coutp * k2;
    RIB_KLAUNCH(k_wino_filters_1x1, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, h->d_blob + h->convs[ws.aux].w_off, ws.d, c.coutp, k2, ws.wm, c.cinp + k2, c.cinp);
    HIP_TRY(h, hipGetLastError());
  }
  return RIB_OK;
}

// index of the F(wm x wm) filter set of conv `ci`, created on first use (plan build): device memory + the transform when the
// weights are already there.  Synchronises the device (before and after the transform) once per new set: plan builds are
// one-time work, and include/rib.h says so for every entry point that can build a plan.  < 0: error (h->err).
int ensure_wino_set(rib_handle* h, int ci, int wm, int aux = -1) {
  auto it = h->wino_index.find({ci, wm, aux});
  if (it != h->wino_index.end()) return it->second;
  const ConvDef& c = h->convs[ci];
  rib_handle::WinoSet ws; ws.conv = ci; ws.wm = wm; ws.aux = aux;
  ws.floats = (size_t)(wm + 2) * (wm + 2) * c.coutp * (c.cinp + (aux >= 0 ? h->convs[aux].cinp : 0));
  if (h->device >= 0) {
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&ws.d), ws.floats * sizeof(float));
    if (e != hipSuccess) { h->err = fmt("Winograd filter set of %s: %s", c.name.c_str(), hipGetErrorString(e)); return -1; }
  }
  const int si = (int)h->wino_sets.size();
  h->wino_sets.push_back(ws);
  h->wino_index[{ci, wm, aux}] = si;
  if (h->device >= 0 && h->weights_ready) {
    // the blob may still be landing on a (non-blocking) stream of the caller's - rib_import_weights returns behind an
    // asynchronous copy - and the NULL stream does not order against such a stream: drain the device first, then transform
    if (hipDeviceSynchronize() != hipSuccess) { h->err = "Winograd filter transform: device not idle-able"; return -1; }
    if (fill_wino_set(h, si, nullptr) != RIB_OK) return -1;
    if (hipDeviceSynchronize() != hipSuccess) { h->err = "Winograd filter transform failed"; return -1; }
  }
  return si;
}

// after the blob changed (finalize / import): every existing set again, on `st`
int refresh_wino_sets(rib_handle* h, hipStream_t st) {
  for (int si = 0; si < (int)h->wino_sets.size(); ++si) {
    const int rc = fill_wino_set(h, si, st);
    if (rc) return rc;
  }
  return RIB_OK;
}
void free_wino_sets(rib_handle* h) {
  for (auto& ws : h->wino_sets) if (ws.d) (void)hipFree(ws.d);
  h->wino_sets.clear(); h->wino_index.clear();
}

// ------------------------------------------------------------------------------------------
// weight layout: sizes are fixed by the config, so offsets are assigned at create time
// ------------------------------------------------------------------------------------------
// k_conv_lowc instantiations: (channels rounded up to the MFMA's k-group, output columns)
static bool lowc_instantiated(int ce, int ncol) {
  return (ce == 6 && ncol == 64) || (ce == 10 && ncol == 32) || (ce == 22 && ncol == 32) || (ce == 24 && ncol == 16);
}
// (fp32 storage only: the 16-bit modes pack their inputs and run the first layers on the 16-bit matrix cores)
template <int CE, int NCOL> static void launch_lowc_t(int tw, dim3 grid, hipStream_t st, const LowcParams& p) {
  if (tw == 16) RIB_KLAUNCH((k_conv_lowc<CE, NCOL, ST_F32, 16>), grid, dim3(256), 0, st, p);
  else RIB_KLAUNCH((k_conv_lowc<CE, NCOL, ST_F32, 32>), grid, dim3(256), 0, st, p);
}
// the Winograd input transform of tile M: staged (k_wino_in_staged) or not, by source mode and second-source mode
template <int M, bool STAGED, int MODE, int MODE2 = -1> static void launch_wino_in_t(dim3 grid, hipStream_t st, const WinoInParams& p) {
  if constexpr (STAGED) RIB_KLAUNCH((k_wino_in_staged<M, MODE, MODE2>), grid, dim3(256), 0, st, p);
  else if constexpr (M == 4) RIB_KLAUNCH((k_wino4_in<MODE, MODE2>), grid, dim3(256), 0, st, p);
  else RIB_KLAUNCH((k_wino_in<MODE, MODE2>), grid, dim3(256), 0, st, p);
}
template <int M, bool STAGED> static void launch_wino_in(const Op& op, hipStream_t st, const WinoInParams& p) {
  if (op.wi_mode2 >= 0) {      // with the shortcut's input as a second source
    const bool s1 = op.wi_mode == WSRC_SPADE, s2 = op.wi_mode2 == WSRC_SPADE;
    if (s1 && s2) launch_wino_in_t<M, STAGED, WSRC_SPADE, WSRC_SPADE>(op.grid, st, p);
    else if (s1) launch_wino_in_t<M, STAGED, WSRC_SPADE, WSRC_PLAIN>(op.grid, st, p);
    else if (s2) launch_wino_in_t<M, STAGED, WSRC_PLAIN, WSRC_SPADE>(op.grid, st, p);
    else launch_wino_in_t<M, STAGED, WSRC_PLAIN, WSRC_PLAIN>(op.grid, st, p);
  } else if (op.wi_mode == WSRC_SPADE) launch_wino_in_t<M, STAGED, WSRC_SPADE>(op.grid, st, p);
  else if (op.wi_mode == WSRC_JOIN) launch_wino_in_t<M, STAGED, WSRC_JOIN>(op.grid, st, p);
  else launch_wino_in_t<M, STAGED, WSRC_PLAIN>(op.grid, st, p);
}

static void launch_lowc(int ce, int ncol, int tw, dim3 grid, hipStream_t st, const LowcParams& p) {
  if (ce == 6 && ncol == 64) launch_lowc_t<6, 64>(tw, grid, st, p);
  else if (ce == 10 && ncol == 32) launch_lowc_t<10, 32>(tw, grid, st, p);
  else if (ce == 22 && ncol == 32) launch_lowc_t<22, 32>(tw, grid, st, p);
  else if (ce == 24 && ncol == 16) launch_lowc_t<24, 16>(tw, grid, st, p);
}

// The blob starts with a header the importer checks (rib_import_weights): a blob is only meaningful to a handle with
// the same precision mode and the same layout (which also depends on RIB_NO_WINO / RIB_NO_LOWC / RIB_NO_SPADE16 as read
// when the layout was assigned).  64 floats are reserved; 8 words are used.
enum { BLOB_HEADER_FLOATS = 64, BLOB_MAGIC = 0x57424952 /* "RIBW" */, BLOB_VERSION = 3 };
struct BlobHeader { uint32_t magic, version, prec, reserved; uint64_t floats, layout_hash; };

void assign_weight_layout(rib_handle* h) {
  size_t off = BLOB_HEADER_FLOATS;
  h->spades.clear(); h->spade_index.clear();
  auto take = [&](size_t nfloats) { size_t o = off; off += (nfloats + 63) / 64 * 64; return o; };
  h->zero_off = take(64);
  for (auto& c : h->convs) {
    if (!c.used) continue;
    c.cinp = h->padc(c.cin);
    c.coutp = pad32(c.cout);
    c.w16_off = c.wp16_off = 0; c.fb_off = 0;
    c.w_off = take((size_t)c.coutp * c.ks * c.ks * c.cinp);
    if (c.ups_in) c.wp_off = take((size_t)c.coutp * 16 * c.cinp);
    c.b_off = take(c.coutp);
    if (c.in_affine) { c.g_off = take(c.coutp); c.be_off = take(c.coutp); }
    if (c.spade_cond && c.name.size() > 13 && c.name.compare(c.name.size() - 13, 13, ".conv_block_1") == 0 &&
        h->conv_index.count(c.name.substr(0, c.name.size() - 1) + "s"))
      c.fb_off = take(c.coutp);
  }
  // SPADE groups: block_0 (+ block_s when the shortcut is learned) share one launch.  Created level by level, in the
  // order the forward runs them (down_i, res_*, up_i), and their filters taken back to back: the filter matrices of a
  // level's groups form ONE [sum npad][cond] matrix in the blob (SpadeGroup::col0)
  {
    const rib_config& gc = h->g.c;
    const int D = gc.num_down_img;
    std::vector<std::pair<std::string, int>> blocks;      // (block name, condition level) in execution order
    for (int i = 0; i <= D; ++i) blocks.push_back({"down_" + std::to_string(i), std::min(gc.emb_down, i)});
    for (int i = 0; i < h->g.num_res_blocks(); ++i) blocks.push_back({"res_" + std::to_string(i), std::min(gc.emb_down, D + 1)});
    for (int i = D; i >= 0; --i) blocks.push_back({"up_" + std::to_string(i), std::min(i, gc.emb_down)});
    h->level_groups.clear();
    for (int level = 0; level <= gc.emb_down; ++level) {
      int col = 0;
      for (auto& bl : blocks) {
        if (bl.second != level) continue;
        for (const char* which : {"0", "1"}) {
          auto it = h->conv_index.find(bl.first + ".conv_block_" + which);
          if (it == h->conv_index.end()) continue;
          const ConvDef& c = h->convs[it->second];
          if (!c.used || !c.spade_cond) continue;
          SpadeGroup sg;
          sg.C = c.cin; sg.Cp = h->padc(c.cin); sg.cond = c.spade_cond;
          sg.nsets = (which[0] == '0' && h->conv_index.count(bl.first + ".conv_block_s")) ? 2 : 1;
          sg.key = bl.first + "." + which;
          sg.npad = (sg.nsets * sg.Cp + 31) / 32 * 64;
          sg.level = level; sg.col0 = col; col += sg.npad;
          sg.w_off = take((size_t)sg.npad * h->padc(sg.cond));      // (a multiple of 64 floats: no gap between two groups)
          h->level_groups[level].push_back((int)h->spades.size());
          h->spade_index[sg.key] = (int)h->spades.size();
          h->spades.push_back(sg);
        }
      }
    }
    for (auto& sg : h->spades) sg.b_off = take(sg.npad);
  }
  for (auto& c : h->convs) { c.wino_ok = false; c.wino_s_ok = false; c.zero_off = 0; }
  if (h->prec() == PREC_F32 && !getenv("RIB_NO_WINO")) {
    // 3x3 stride-1 convolutions with >= 128 input channels that own their launch (no fused 1x1 shortcut, no upsampled
    // input): the deep residual blocks of the generator and of the mask network
    for (auto& c : h->convs) {
      // (measured per layer at 512x512, transforms included: 512->512 at 32x32 58 -> 38 us, 256->256 at 64x64 47-52 -> 42 us,
      // 512->256 at 64x64 95 -> 63 us; 128->128 at 64x64 gains nothing: the two transforms cost ~13 us per layer)
      // (with a fused 1x1 shortcut: eligible at any width - only a measured table entry switches such a layer over)
      if (c.used && c.ks == 3 && c.stride == 1 && !c.ups_in && c.fb_off != 0 && c.cout >= 64 && c.cinp % 32 == 0 && 128 % (c.coutp / 4) == 0) c.wino_s_ok = true;
      if (!c.used || c.ks != 3 || c.stride != 1 || c.ups_in || c.fb_off != 0 || c.cin < 256 || c.cout < 64 || c.cinp % 32 || 128 % (c.coutp / 4)) continue;
      // the plan picks F(4x4) or F(2x2) per layer from the map size (conv_wino) and asks for that filter set then
      c.wino_ok = true;
      c.zero_off = take(c.coutp);
    }
  }
  for (auto& sg : h->spades) {
    sg.w1_off = sg.b1_off = 0;
    if (h->prec() == PREC_F32 && sg.nsets * sg.Cp == 16 && !getenv("RIB_NO_SPADE16")) {
      sg.w1_off = take((size_t)32 * h->padc(sg.cond));
      sg.b1_off = take(32);
    }
  }
  // first-layer convolutions over the caller's tensors (k_conv_lowc, fp32 arithmetic): filter in real-channel K order.  Not
  // with bf16 storage: there the packed bf16 copy + bf16 matrix cores are faster (679 vs 672 frames/s, A/B)
  for (auto& c : h->convs) {
    c.wl_off = 0; c.lowc_ce = c.lowc_ncol = 0;
    if (!c.used || c.ks != 3 || c.stride != 1 || c.ups_in || c.fb_off != 0 || c.cin > 24 || h->mc16() || getenv("RIB_NO_LOWC")) continue;
    const int ncol = c.cout <= 16 ? 16 : c.coutp;      // (coutp is a multiple of 32; the 16-column instantiation serves Cout <= 16)
    const int ce = ncol == 16 ? (c.cin + 3) / 4 * 4 : (c.cin + 1) / 2 * 2;
    if (!lowc_instantiated(ce, ncol)) continue;
    c.lowc_ce = ce; c.lowc_ncol = ncol;
    c.wl_off = take((size_t)9 * ce * ncol);
  }
  if (h->mc16()) {   // bf16 copies of every filter tensor the matrix-core kernels read (two elements per float)
    const size_t pl = 1;
    for (auto& c : h->convs) {
      if (!c.used) continue;
      c.w16_off = take((pl * c.coutp * c.ks * c.ks * c.cinp + 1) / 2);
      if (c.ups_in) c.wp16_off = take((pl * c.coutp * 16 * c.cinp + 1) / 2);
    }
    for (auto& sg : h->spades) sg.w16_off = take((pl * sg.npad * h->padc(sg.cond) + 1) / 2);
  }
  h->blob_floats = off;
  // FNV-1a over every offset the kernels will be handed
  uint64_t hs = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { for (int i = 0; i < 8; ++i) { hs ^= (v >> (8 * i)) & 0xff; hs *= 1099511628211ull; } };
  for (const auto& c : h->convs)
    for (uint64_t v : {(uint64_t)c.w_off, (uint64_t)c.b_off, (uint64_t)c.g_off, (uint64_t)c.be_off, (uint64_t)c.fb_off, (uint64_t)c.wp_off, (uint64_t)c.w16_off,
                       (uint64_t)c.wp16_off, (uint64_t)c.zero_off, (uint64_t)c.wl_off}) mix(v);
  for (const auto& sg : h->spades)
    for (uint64_t v : {(uint64_t)sg.w_off, (uint64_t)sg.b_off, (uint64_t)sg.w16_off, (uint64_t)sg.w1_off, (uint64_t)sg.b1_off}) mix(v);
  mix(off);
  h->layout_hash = hs;
}
BlobHeader blob_header_of(const rib_handle* h) {
  BlobHeader bh; bh.magic = BLOB_MAGIC; bh.version = BLOB_VERSION; bh.prec = (uint32_t)h->prec(); bh.reserved = 0;
  bh.floats = h->blob_floats; bh.layout_hash = h->layout_hash;
  return bh;
}

void register_tensors(rib_handle* h) {
  auto add = [&](const std::string& n, std::vector<int64_t> d, bool used) {
    TensorDef t; t.name = n; t.dims = d; t.used = used;
    h->tensor_index[n] = (int)h->tensors.size();
    h->tensors.push_back(t);
  };
  for (auto& c : h->convs) {
    if (c.spade_cond) {
      add(c.name + ".layers.norm.mlps.0.0.layers.conv.weight", {2 * c.cin, c.spade_cond, 1, 1}, c.used);
      add(c.name + ".layers.norm.mlps.0.0.layers.conv.bias", {2 * c.cin}, c.used);
    }
    const std::string p = c.name + ".layers.conv";
    if (c.spectral) {
      add(p + ".bias", {c.cout}, c.used);
      add(p + ".weight_orig", {c.cout, c.cin, c.ks, c.ks}, c.used);
      add(p + ".weight_u", {c.cout}, c.used);
      add(p + ".weight_v", {(int64_t)c.cin * c.ks * c.ks}, c.used);
    } else {
      add(p + ".weight", {c.cout, c.cin, c.ks, c.ks}, c.used);
      add(p + ".bias", {c.cout}, c.used);
    }
    if (c.in_affine) {
      add(c.name + ".layers.norm.weight", {c.cout}, c.used);
      add(c.name + ".layers.norm.bias", {c.cout}, c.used);
    }
  }
}

const std::vector<float>* tensor_data(rib_handle* h, const std::string& name) {
  auto it = h->tensor_index.find(name);
  if (it == h->tensor_index.end()) return nullptr;
  TensorDef& t = h->tensors[it->second];
  return t.set ? &t.data : nullptr;
}

}  // namespace

#include "planner.h"      // FusionPolicy, Builder: a shape -> a Plan

namespace {

// PLAN_LABELS: the label-only launches alone (rib_chain's batched pre-pass).  PLAN_UNPAIRED: a frame plan that keeps the mask
// network's label encoder in launches of its own (rib_chain skips them); the default frame plan pairs the two encoders
// level by level at batch 1 (Builder::mask_branches_paired) - same kernels, same choices, bit-identical frames.
enum { PLAN_LABELS = 1, PLAN_UNPAIRED = 2 };
inline bool plan_pairs(int B, int flags) {
  return FusionPolicy::pair_mask_encoders() && B == 1 && !(flags & (PLAN_LABELS | PLAN_UNPAIRED));
}
Plan* get_plan(rib_handle* h, int B, int H, int W, int flags = 0, int tuneB = 0) {
  const bool labels_only = (flags & PLAN_LABELS) != 0;
  if (!labels_only && !plan_pairs(B, 0)) flags &= ~PLAN_UNPAIRED;      // one frame plan where nothing is paired anyway
  if (h->plan_batch > 0) tuneB = h->plan_batch;                       // batch-invariant policy (rib_set_plan_batch)
  if (tuneB == B) tuneB = 0;
  const std::array<int, 5> key = {flags & 3, tuneB, B, H, W};
  auto it = h->plans.find(key);
  if (it != h->plans.end()) return it->second.get();
  const int mult = 1 << std::max(h->g.c.num_down_img, h->g.c.mask_down);
  if (B < 1 || H < mult || W < mult || H % mult || W % mult) {
    h->err = fmt("unsupported shape B=%d H=%d W=%d: H and W must be positive multiples of %d (SURVEY F5)", B, H, W, mult);
    return nullptr;
  }
  {  // the kernels address one sample with 32-bit element offsets: H*W*C < 2^31 for every activation
    const rib_config& c = h->g.c;
    const size_t widest = (size_t)std::max(std::max(c.emb_filters, c.mask_filters * 2), std::max(c.num_filters * 2, 32));
    if ((size_t)H * W * widest >= (1ull << 31)) {
      h->err = fmt("unsupported shape H=%d W=%d: a full-resolution activation exceeds 2^31 elements", H, W);
      return nullptr;
    }
  }
  std::unique_ptr<Plan> P(new Plan());
  P->B = B; P->H = H; P->W = W;
  Builder b; b.h = h; b.P = P.get(); b.B = B; b.tuneB = tuneB; b.pair_mask = plan_pairs(B, flags);
  if (!(labels_only ? b.build_labels() : b.build())) { h->err = "plan: " + b.error; return nullptr; }
  Plan* raw = P.get();
  h->plans[key] = std::move(P);
  return raw;
}

// ------------------------------------------------------------------------------------------
// launch
// ------------------------------------------------------------------------------------------
struct Resolver {
  char* ws; float* blob; const void* user[U_COUNT];
  const rib_handle* h = nullptr;     // for PS_WINO
  void* get(const PRef& r) const {
    switch (r.sp) {
      case PS_WS: return ws + r.off;
      case PS_WEIGHT: return blob + r.off;
      case PS_WINO: return h->wino_sets[r.off].d;
      case PS_USER: return const_cast<void*>(user[r.off]);
      default: return nullptr;
    }
  }
};

// a kernel templated on the storage type alone, launched for the handle's precision mode
#define RIB_LAUNCH_ST(prec, KERNEL, grid, block, lds, st, ...)                                                        \
  do {                                                                                                                \
    if ((prec) == PREC_BF16) RIB_KLAUNCH((KERNEL<ST_BF16>), grid, block, lds, st, __VA_ARGS__);                \
    else if ((prec) == PREC_F16) RIB_KLAUNCH((KERNEL<ST_F16>), grid, block, lds, st, __VA_ARGS__);             \
    else RIB_KLAUNCH((KERNEL<ST_F32>), grid, block, lds, st, __VA_ARGS__);                                     \
  } while (0)

template <int CO, int CIN> void launch_head_t(int bf16, dim3 grid, hipStream_t st, const IgemmParams& p) {
  if (bf16 == PREC_BF16) RIB_KLAUNCH((k_conv_head<CO, CIN, ST_BF16>), grid, dim3(256), 0, st, p);
  else if (bf16 == PREC_F16) RIB_KLAUNCH((k_conv_head<CO, CIN, ST_F16>), grid, dim3(256), 0, st, p);
  else RIB_KLAUNCH((k_conv_head<CO, CIN, ST_F32>), grid, dim3(256), 0, st, p);
}
template <int CO> void launch_small_t(int bf16, dim3 grid, size_t lds, hipStream_t st, const IgemmParams& p) {
  if (bf16 == PREC_BF16) RIB_KLAUNCH((k_conv_small<CO, ST_BF16>), grid, dim3(256), lds, st, p);
  else if (bf16 == PREC_F16) RIB_KLAUNCH((k_conv_small<CO, ST_F16>), grid, dim3(256), lds, st, p);
  else RIB_KLAUNCH((k_conv_small<CO, ST_F32>), grid, dim3(256), lds, st, p);
}
void launch_head(int co, int cin, int bf16, dim3 grid, hipStream_t st, const IgemmParams& p) {
  if (cin == 16) { if (co == 1) launch_head_t<1, 16>(bf16, grid, st, p); else if (co == 2) launch_head_t<2, 16>(bf16, grid, st, p); else launch_head_t<3, 16>(bf16, grid, st, p); }
  else { if (co == 1) launch_head_t<1, 32>(bf16, grid, st, p); else if (co == 2) launch_head_t<2, 32>(bf16, grid, st, p); else launch_head_t<3, 32>(bf16, grid, st, p); }
}

int run_plan(rib_handle* h, Plan* P, const Resolver& R, hipStream_t st, bool skip_label_ops = false) {
  const int bf16 = h->prec();       // storage type of the activations: PREC_F32 / PREC_BF16 / PREC_F16
  for (Op& op : P->ops) {
    if (skip_label_ops && op.label_only) continue;     // done for the whole chain by the labels-only plan
    g_prof_pair = ProfPair();
    if (h->profiling && h->prof_kernels) {      // the launch below carries its own (start, stop) pair
      ProfPair pp;
      HIP_TRY(h, hipEventCreate(&pp.start));
      HIP_TRY(h, hipEventCreate(&pp.stop));
      h->prof_kernel_events.push_back({op.kclass, pp.start, pp.stop});
      g_prof_pair = pp;
    } else if (h->profiling) {      // one event in front of every launch (rib.h: a launch is charged the time to the next event)
      hipEvent_t e0 = nullptr;
      HIP_TRY(h, hipEventCreate(&e0));
      HIP_TRY(h, hipEventRecord(e0, st));
      h->prof_events.push_back({op.kclass, e0});
    }
    // the launch's own copy of its parameters: scalars as planned, every bound pointer resolved
    OpParams params = op.params;
    for (int i = 0; i < op.nbinds; ++i) {
      void* ptr = R.get(op.binds[i].ref);
      memcpy(reinterpret_cast<char*>(&params) + op.binds[i].field, &ptr, sizeof ptr);
    }
    switch (op.kind()) {
      case OP_IGEMM: {
        IgemmParams& p = std::get<IgemmParams>(params);
        p.zeros = R.blob + h->zero_off;
        if (op.small_co > 0 && op.head) {
          if (op.fuse_blend && R.user[U_FUSE]) {
            p.bl_img = reinterpret_cast<const float*>(R.user[U_IMG]); p.bl_dain = reinterpret_cast<const float*>(R.user[U_FAKE]);
            p.bl_fuse = reinterpret_cast<float*>(const_cast<void*>(R.user[U_FUSE]));
          }
          launch_head(op.small_co, p.Cin, bf16, op.grid, st, p);
        } else if (op.small_co > 0) {
          const size_t lds = ((size_t)18 * 18 * (p.Cin + 4) + (size_t)op.small_co * 9 * p.Cin) * sizeof(float);
          switch (op.small_co) {
            case 1: launch_small_t<1>(bf16, op.grid, lds, st, p); break;
            case 2: launch_small_t<2>(bf16, op.grid, lds, st, p); break;
            case 3: launch_small_t<3>(bf16, op.grid, lds, st, p); break;
            default: launch_small_t<4>(bf16, op.grid, lds, st, p); break;
          }
        } else
        RIB_KLAUNCH(pick_igemm_fn(op.var, p), op.grid, dim3(256 * op.var->KW), 0, st, p);
      } break;
      case OP_GEMM:
        RIB_KLAUNCH(h->products == RIB_PRODUCTS_BF16X3 && op.var->gfn_x3 ? op.var->gfn_x3 : op.var->gfn, op.grid, dim3(256), 0, st, std::get<GemmDmaParams>(params));
        break;
      case OP_FINALIZE: {
        const FinalizeParams& p = std::get<FinalizeParams>(params);
        if (p.tiles > 512) RIB_KLAUNCH(k_stats_finalize<4>, dim3((p.Cs + 3) / 4, op.grid.y, op.grid.z), dim3(1024), 0, st, p);
        else RIB_KLAUNCH(k_stats_finalize<16>, op.grid, dim3(1024), 0, st, p);
      } break;
      case OP_MODULATE: RIB_LAUNCH_ST(bf16, k_spade_modulate, op.grid, dim3(256), 0, st, std::get<ModulateParams>(params)); break;
      case OP_SPLITEPI: RIB_LAUNCH_ST(bf16, k_splitk_epilogue, op.grid, dim3(256), 0, st, std::get<SplitEpiParams>(params)); break;
      case OP_POOL: RIB_LAUNCH_ST(bf16, k_avgpool, op.grid, dim3(256), 0, st, std::get<PoolParams>(params)); break;
      case OP_INADD: RIB_LAUNCH_ST(bf16, k_in_add, op.grid, dim3(256), 0, st, std::get<InAddParams>(params)); break;
      case OP_WINO_IN:
        if (op.wino_m == 4) { if (op.wi_staged) launch_wino_in<4, true>(op, st, std::get<WinoInParams>(params)); else launch_wino_in<4, false>(op, st, std::get<WinoInParams>(params)); }
        else { if (op.wi_staged) launch_wino_in<2, true>(op, st, std::get<WinoInParams>(params)); else launch_wino_in<2, false>(op, st, std::get<WinoInParams>(params)); }
        break;
      case OP_WINO_OUT:
        if (op.wino_m == 4) RIB_KLAUNCH(k_wino4_out, op.grid, dim3(256), 0, st, std::get<WinoOutParams>(params));
        else RIB_KLAUNCH(k_wino_out, op.grid, dim3(256), 0, st, std::get<WinoOutParams>(params));
        break;
      case OP_LOWC: launch_lowc(op.lowc_ce, op.lowc_ncol, op.lowc_tw, op.grid, st, std::get<LowcParams>(params)); break;
      case OP_PACK: RIB_LAUNCH_ST(bf16, k_pack, op.grid, dim3(256), 0, st, std::get<PackParams>(params)); break;
    }
  }
  g_prof_pair = ProfPair();
  if (h->profiling && !h->prof_kernels) {        // closes the last launch's interval
    hipEvent_t e1 = nullptr;
    HIP_TRY(h, hipEventCreate(&e1));
    HIP_TRY(h, hipEventRecord(e1, st));
    h->prof_events.push_back({-1, e1});
  }
  HIP_TRY(h, hipGetLastError());
  return RIB_OK;
}

int check_ready(rib_handle* h) {
  if (!h) return RIB_ERR_INVALID;
  if (!h->weights_ready) return fail(h, RIB_ERR_STATE, "weights not loaded: call rib_finalize_weights() or rib_import_weights() first");
  return RIB_OK;
}

}  // namespace

// ==========================================================================================
// C ABI
// ==========================================================================================
extern "C" {

int rib_create(const rib_config* cfg, int device, rib_handle** out) {
  if (!cfg || !out) { g_create_error = "rib_create: null argument"; return RIB_ERR_INVALID; }
  *out = nullptr;
  const rib_config& c = *cfg;
  auto bad = [&](const std::string& m) { g_create_error = "rib_create: " + m; return RIB_ERR_UNSUPPORTED; };
  if (c.label_nc < 1 || c.image_nc < 1 || c.num_filters < 1 || c.num_down_img < 1 || c.mask_down < 1 ||
      c.emb_filters < 1 || c.mask_filters < 1 || c.mask_res_blocks < 1 || c.num_layers < c.num_down_img)
    return bad("invalid hyper-parameters");
  if (c.emb_down != c.num_down_img) return bad("embed.num_downsamples must equal num_downsamples_img (HSM.yaml: 4/4)");
  std::unique_ptr<rib_handle> h(new rib_handle());
  h->g.c = c; h->device = device; h->label_nc = c.label_nc;
  h->graph_replay = getenv("RIB_GRAPH") != nullptr && atoi(getenv("RIB_GRAPH")) != 0;
  h->wino_in_staging = !(getenv("RIB_WINO_IN_UNSTAGED") != nullptr && atoi(getenv("RIB_WINO_IN_UNSTAGED")) != 0);
  for (int i = 0; i <= c.emb_down; ++i) {
    if (h->g.cond_ch(i) != h->g.emb_ch(i)) return bad("embed/generator max_num_filters disagree on the cond map width");
    if (h->g.emb_ch(i) % 32 != 0) return bad(fmt("embed width %d at level %d is not a multiple of 32", h->g.emb_ch(i), i));
  }
  for (int i = 1; i <= c.mask_down; ++i)
    if (h->g.mask_nf(i - 1) % 32 != 0) return bad("mask.num_filters must be a multiple of 32 (stride-2 kernels use 32-channel chunks)");
  for (int i = 0; i <= c.num_down_img + 1; ++i) {
    const int ch = h->g.nf(i);
    if (ch % 4 != 0 || 256 % (ch / 4 > 0 ? ch / 4 : 1) != 0 || ch > 1024) return bad(fmt("generator width %d unsupported (power-of-two multiples of 4 up to 1024)", ch));
  }
  h->convs = build_inventory(h->g);
  for (size_t i = 0; i < h->convs.size(); ++i) h->conv_index[h->convs[i].name] = (int)i;
  register_tensors(h.get());
  assign_weight_layout(h.get());
  if (device >= 0) {   // device < 0: host-only handle (inventory, plans, weight fold; no launches)
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->d_blob), h->blob_floats * sizeof(float));
    h->d_blob_floats = h->blob_floats;
    if (e != hipSuccess) { g_create_error = fmt("rib_create: device %d: %s", device, hipGetErrorString(e)); return RIB_ERR_HIP; }
  }
  *out = h.release();
  return RIB_OK;
}

void rib_destroy(rib_handle* h) {
  if (!h) return;
  drop_chain_graphs(h);
  h->stage.release();
  h->png.release();
  if (h->d_blob) (void)hipFree(h->d_blob);
  free_wino_sets(h);
  for (auto& pe : h->prof_events) (void)hipEventDestroy(pe.second);
  for (auto& ke : h->prof_kernel_events) { (void)hipEventDestroy(ke.start); (void)hipEventDestroy(ke.stop); }
  delete h;
}

const char* rib_last_error(const rib_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int rib_num_tensors(const rib_handle* h) { return h ? (int)h->tensors.size() : RIB_ERR_INVALID; }

int rib_tensor_info(const rib_handle* h, int idx, const char** name, int* ndim, int64_t dims[4], int* used) {
  if (!h || idx < 0 || idx >= (int)h->tensors.size()) return RIB_ERR_INVALID;
  const TensorDef& t = h->tensors[idx];
  if (name) *name = t.name.c_str();
  if (ndim) *ndim = (int)t.dims.size();
  if (dims) for (size_t i = 0; i < 4; ++i) dims[i] = i < t.dims.size() ? t.dims[i] : 1;
  if (used) *used = t.used ? 1 : 0;
  return RIB_OK;
}

int rib_set_tensor(rib_handle* h, const char* name, const float* data, int ndim, const int64_t* dims) {
  if (!h || !name || !data || !dims) return RIB_ERR_INVALID;
  auto it = h->tensor_index.find(name);
  if (it == h->tensor_index.end()) return fail(h, RIB_ERR_INVALID, fmt("unexpected key '%s' in state_dict (strict load, PGNR/utils/utils.py:119)", name));
  TensorDef& t = h->tensors[it->second];
  if (ndim != (int)t.dims.size()) return fail(h, RIB_ERR_INVALID, fmt("'%s': rank %d, expected %zu", name, ndim, t.dims.size()));
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (dims[i] != t.dims[i]) return fail(h, RIB_ERR_INVALID, fmt("size mismatch for '%s' (dim %d: %lld vs %lld)", name, i, (long long)dims[i], (long long)t.dims[i]));
    n *= (size_t)dims[i];
  }
  if (t.used) t.data.assign(data, data + n);   // tensors of never-called modules are accepted and dropped
  t.set = true;
  h->weights_ready = false;
  return RIB_OK;
}

int rib_finalize_weights(rib_handle* h) {
  if (!h) return RIB_ERR_INVALID;
  for (auto& t : h->tensors)
    if (!t.set) return fail(h, RIB_ERR_MISSING, fmt("missing key '%s' in state_dict (strict load)", t.name.c_str()));
  std::vector<float> blob(h->blob_floats, 0.f);
  { const BlobHeader bh = blob_header_of(h); memcpy(blob.data(), &bh, sizeof bh); }
  for (auto& c : h->convs) {
    if (!c.used) continue;
    const std::string p = c.name + ".layers.conv";
    const int K = c.cin * c.ks * c.ks;
    const std::vector<float>* w = nullptr;
    double sigma = 1.0;
    if (c.spectral) {
      w = tensor_data(h, p + ".weight_orig");
      const std::vector<float>& u = *tensor_data(h, p + ".weight_u");
      const std::vector<float>& v = *tensor_data(h, p + ".weight_v");
      // sigma = u . (W_mat v): eval-mode spectral norm, u and v exactly as stored
      double s = 0.0;
      for (int o = 0; o < c.cout; ++o) {
        double row = 0.0;
        for (int k = 0; k < K; ++k) row += (double)(*w)[(size_t)o * K + k] * (double)v[k];
        s += (double)u[o] * row;
      }
      sigma = s;
      if (sigma == 0.0 || !std::isfinite(sigma)) return fail(h, RIB_ERR_INVALID, fmt("'%s': spectral norm sigma is %g", c.name.c_str(), sigma));
    } else {
      w = tensor_data(h, p + ".weight");
    }
    const std::vector<float>& b = *tensor_data(h, p + ".bias");
    const float inv = (float)sigma;
    const int taps = c.ks * c.ks;
    // OIHW -> [CoutPad][tap][CinPad]; torch computes weight_orig / sigma in fp32
    for (int o = 0; o < c.cout; ++o)
      for (int i = 0; i < c.cin; ++i)
        for (int t = 0; t < taps; ++t) {
          const float wv = (*w)[((size_t)o * c.cin + i) * taps + t];
          blob[c.w_off + ((size_t)o * taps + t) * c.cinp + i] = c.spectral ? wv / inv : wv;
        }
    for (int o = 0; o < c.cout; ++o) blob[c.b_off + o] = b[o];
    if (c.ups_in) {
      // phase filters of the upsample convolution (k_igemm, UPS): along each axis, phase p and tap a
      // sum the original taps   p = 0: a = 0 <- {0}, a = 1 <- {1, 2};   p = 1: a = 0 <- {0, 1}, a = 1 <- {2}
      // (fp32 sums of the folded filters, in a fixed dy-major order)
      static const int lo[2][2] = {{0, 1}, {0, 2}}, hi[2][2] = {{0, 2}, {1, 2}};   // [p][a]: inclusive tap range
      for (int o = 0; o < c.cout; ++o)
        for (int ph = 0; ph < 4; ++ph)
          for (int a = 0; a < 2; ++a)
            for (int bb = 0; bb < 2; ++bb) {
              const int py = ph >> 1, px = ph & 1;
              float* dst = &blob[c.wp_off + ((size_t)o * 16 + ph * 4 + a * 2 + bb) * c.cinp];
              for (int i = 0; i < c.cin; ++i) {
                float acc = 0.f;
                for (int dy = lo[py][a]; dy <= hi[py][a]; ++dy)
                  for (int dx = lo[px][bb]; dx <= hi[px][bb]; ++dx)
                    acc += blob[c.w_off + ((size_t)o * 9 + dy * 3 + dx) * c.cinp + i];
                dst[i] = acc;
              }
            }
    }
    if (c.in_affine) {
      const std::vector<float>& gm = *tensor_data(h, c.name + ".layers.norm.weight");
      const std::vector<float>& bt = *tensor_data(h, c.name + ".layers.norm.bias");
      for (int o = 0; o < c.cout; ++o) { blob[c.g_off + o] = gm[o]; blob[c.be_off + o] = bt[o]; }
    }
  }
  for (auto& c : h->convs) {
    if (!c.used || !c.fb_off) continue;
    const ConvDef& cs = conv_of(h, c.name.substr(0, c.name.size() - 1) + "s");
    for (int o = 0; o < c.cout; ++o) blob[c.fb_off + o] = blob[c.b_off + o] + blob[cs.b_off + o];
  }
  // SPADE gamma/beta filters: virtual column pairs [gamma(32) | beta(32)] per 32 virtual channels;
  // virtual channel v = set*Cp + c, set 0 = conv_block_0/1, set 1 = conv_block_s
  for (auto& sg : h->spades) {
    const std::string blk = sg.key.substr(0, sg.key.size() - 2);
    const std::string which = sg.key.substr(sg.key.size() - 1);
    const int condp = h->padc(sg.cond);
    for (int set = 0; set < sg.nsets; ++set) {
      const std::string cn = blk + ".conv_block_" + (set == 0 ? which : std::string("s"));
      const std::string sp = cn + ".layers.norm.mlps.0.0.layers.conv";
      const std::vector<float>& w = *tensor_data(h, sp + ".weight");   // [2C][cond]
      const std::vector<float>& b = *tensor_data(h, sp + ".bias");
      for (int ch = 0; ch < sg.C; ++ch) {
        const int v = set * sg.Cp + ch;
        const int colg = (v / 32) * 64 + (v % 32), colb = colg + 32;
        for (int k = 0; k < sg.cond; ++k) {
          blob[sg.w_off + (size_t)colg * condp + k] = w[(size_t)ch * sg.cond + k];              // gamma = first C rows
          blob[sg.w_off + (size_t)colb * condp + k] = w[(size_t)(sg.C + ch) * sg.cond + k];     // beta = last C rows
        }
        blob[sg.b_off + colg] = b[ch];
        blob[sg.b_off + colb] = b[sg.C + ch];
        if (sg.w1_off) {   // [gamma(16) | beta(16)]: v < 16
          for (int k = 0; k < sg.cond; ++k) {
            blob[sg.w1_off + (size_t)v * condp + k] = w[(size_t)ch * sg.cond + k];
            blob[sg.w1_off + (size_t)(16 + v) * condp + k] = w[(size_t)(sg.C + ch) * sg.cond + k];
          }
          blob[sg.b1_off + v] = b[ch];
          blob[sg.b1_off + 16 + v] = b[sg.C + ch];
        }
      }
    }
  }
  for (auto& c : h->convs) {
    if (!c.used || !c.wl_off) continue;
    // k_conv_lowc: [step][k within the MFMA's group][column], k = tap * CE + channel over the REAL channels (zero for the
    // channels that round Cin up to the group and for columns beyond Cout)
    const int CE = c.lowc_ce, N = c.lowc_ncol, KG = N == 16 ? 4 : 2;
    for (int k = 0; k < 9 * CE; ++k) {
      const int tap = k / CE, ch = k % CE;
      for (int col = 0; col < N; ++col)
        blob[c.wl_off + (size_t)k * N + col] = (col < c.cout && ch < c.cin) ? blob[c.w_off + ((size_t)col * 9 + tap) * c.cinp + ch] : 0.f;
    }
    (void)KG;   // (step s, slot j) = (k / KG, k % KG): the rows are already in k order
  }
  if (h->mc16()) {
    // rows of `rowlen` K-contiguous elements: [row][rowlen] bf16
    // IEEE half ends at 65504: a folded filter beyond it (a trained checkpoint's W / sigma can be far larger than the seed-defined
    // ones the mode was developed on) would become an infinity in the 16-bit copy and a NaN frame later - refuse it HERE, by name
    std::string out_of_range;
    auto to16 = [&](const std::string& name, size_t src, size_t dst, size_t rows, size_t rowlen) {
      uint16_t* d = reinterpret_cast<uint16_t*>(&blob[dst]);
      if (h->prec() == PREC_F16) {
        for (size_t i = 0; i < rows * rowlen; ++i) {
          const float v = blob[src + i];
          if (!(std::fabs(v) <= 65504.f) && out_of_range.empty()) out_of_range = fmt("%s: folded filter value %g", name.c_str(), (double)v);
          d[i] = host_f16(v);
        }
      } else for (size_t i = 0; i < rows * rowlen; ++i) d[i] = host_bf16(blob[src + i]);
    };
    for (auto& c : h->convs) {
      if (!c.used) continue;
      to16(c.name, c.w_off, c.w16_off, (size_t)c.coutp * c.ks * c.ks, c.cinp);      // a "row" is one (output channel, tap) slice
      if (c.ups_in) to16(c.name, c.wp_off, c.wp16_off, (size_t)c.coutp * 16, c.cinp);
    }
    for (auto& sg : h->spades) to16(sg.key, sg.w_off, sg.w16_off, sg.npad, h->padc(sg.cond));
    if (!out_of_range.empty())
      return fail(h, RIB_ERR_INVALID, "rib_finalize_weights: " + out_of_range + " is outside IEEE half's range (65504): this checkpoint cannot run in "
                                      "RIB_DTYPE_F16; use RIB_DTYPE_BF16 (same speed, fp32's range) or RIB_DTYPE_F32");
  }
  if (h->device < 0) {
    h->host_blob.swap(blob);
  } else {
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->d_blob_floats != h->blob_floats) {
      drop_chain_graphs(h);
      if (h->d_blob) (void)hipFree(h->d_blob);
      h->d_blob = nullptr; h->d_blob_floats = 0;
      HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_blob), h->blob_floats * sizeof(float)));
      h->d_blob_floats = h->blob_floats;
    }
    HIP_TRY(h, hipMemcpy(h->d_blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice));
    h->weights_ready = true;
    const int rcw = refresh_wino_sets(h, nullptr);      // sets that plans already use follow the new weights
    if (rcw) return rcw;
    HIP_TRY(h, hipDeviceSynchronize());
  }
  // the host copies stay (138 MB at HSM.yaml's size): a later rib_set_tensor of a SUBSET of the tensors followed by
  // rib_finalize_weights (load_state_dict(strict=False), a fine-tuned head) folds the new values with the old ones
  return RIB_OK;
}

size_t rib_weights_bytes(const rib_handle* h) { return h ? h->blob_floats * sizeof(float) : 0; }

int rib_export_weights(rib_handle* h, void* dst, size_t bytes, void* hip_stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!dst || bytes != h->blob_floats * sizeof(float)) return fail(h, RIB_ERR_INVALID, "rib_export_weights: size mismatch");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(dst, h->d_blob, bytes, hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(hip_stream)));
  return RIB_OK;
}

int rib_import_weights(rib_handle* h, const void* src, size_t bytes, void* hip_stream) {
  if (!h) return RIB_ERR_INVALID;
  if (!src || bytes != h->blob_floats * sizeof(float)) return fail(h, RIB_ERR_INVALID, "rib_import_weights: size mismatch");
  if (h->device < 0) return fail(h, RIB_ERR_INVALID, "rib_import_weights: host-only handle");
  HIP_TRY(h, hipSetDevice(h->device));
  drop_chain_graphs(h);      // (the blob may move)
  {   // the byte count alone does not identify a layout: check the header (a 32-byte read behind whatever filled src on this stream)
    BlobHeader got;
    HIP_TRY(h, hipMemcpyAsync(&got, src, sizeof got, hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(hip_stream)));
    HIP_TRY(h, hipStreamSynchronize(reinterpret_cast<hipStream_t>(hip_stream)));
    const BlobHeader want = blob_header_of(h);
    if (got.magic != want.magic || got.version != want.version)
      return fail(h, RIB_ERR_INVALID, "rib_import_weights: not a weight blob of this library version (bad header)");
    if (got.prec != want.prec || got.floats != want.floats || got.layout_hash != want.layout_hash)
      return fail(h, RIB_ERR_INVALID, fmt("rib_import_weights: blob was exported by a handle with another precision mode or filter layout "
                                          "(mode %u vs %u, layout hash %016llx vs %016llx)", got.prec, want.prec,
                                          (unsigned long long)got.layout_hash, (unsigned long long)want.layout_hash));
  }
  if (h->d_blob_floats != h->blob_floats) {
    if (h->d_blob) (void)hipFree(h->d_blob);
    h->d_blob = nullptr; h->d_blob_floats = 0;
    HIP_TRY(h, hipMalloc(reinterpret_cast<void**>(&h->d_blob), h->blob_floats * sizeof(float)));
    h->d_blob_floats = h->blob_floats;
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_blob, src, bytes, hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(hip_stream)));
  h->weights_ready = true;
  return refresh_wino_sets(h, reinterpret_cast<hipStream_t>(hip_stream));      // stream-ordered behind the copy
}

int rib_set_compute_dtype(rib_handle* h, int dtype) {
  if (!h || (dtype != RIB_DTYPE_F32 && dtype != RIB_DTYPE_BF16 && dtype != RIB_DTYPE_F16)) return RIB_ERR_INVALID;
  const int mode = dtype == RIB_DTYPE_BF16 ? PREC_BF16 : (dtype == RIB_DTYPE_F16 ? PREC_F16 : PREC_F32);
  if (h->prec_mode == mode) return RIB_OK;
  // The storage type decides the activation / filter layout (bf16: 16-channel minimum, bf16 filter copies in the
  // blob): plans and the weight layout are rebuilt, and the folded blob has to be produced again - by
  // rib_finalize_weights from the state-dict tensors the handle still holds, or by rib_import_weights from a blob
  // exported by a handle of the same storage type.
  h->plans.clear();
  drop_chain_graphs(h);
  free_wino_sets(h);       // (plans reference them by index; the bf16 mode has none)
  h->choices.clear();      // tuned variant indices belong to the previous precision's kernels: back to the cost model until re-pinned
  h->prec_mode = mode;
  assign_weight_layout(h);
  const bool had = h->weights_ready || !h->host_blob.empty();
  h->weights_ready = false;
  h->host_blob.clear();
  if (had) {
    bool all = true;
    for (auto& t : h->tensors) all = all && t.set && (!t.used || !t.data.empty());
    if (all) return rib_finalize_weights(h);
  }
  return RIB_OK;
}

int rib_set_products(rib_handle* h, int products) {
  if (!h || (products != RIB_PRODUCTS_F32 && products != RIB_PRODUCTS_BF16X3)) return RIB_ERR_INVALID;
  if (h->products == products) return RIB_OK;
  drop_chain_graphs(h);      // (captured segments hold the kernels of the other setting)
  h->products = products;
  return RIB_OK;
}

size_t rib_workspace_bytes(rib_handle* h, int B, int H, int W) {
  if (!h) return 0;
  Plan* P = get_plan(h, B, H, W);
  if (!P) return 0;
  size_t need = P->ws_bytes;
  if (plan_pairs(B, 0)) {      // rib_chain runs the unpaired twin of the frame plan on the same workspace
    Plan* PU = get_plan(h, B, H, W, PLAN_UNPAIRED);
    if (!PU) return 0;
    need = std::max(need, PU->ws_bytes);
  }
  // + scratch img/mask frames rib_chain uses when the caller does not ask for them
  return need + 2 * align256((size_t)B * h->g.c.image_nc * H * W * sizeof(float)) +
         align256((size_t)B * H * W * sizeof(float));
}

int rib_forward(rib_handle* h, int B, int H, int W, const float* label, const float* img_fake,
                const float* img_prev, float* img, float* mask, void* workspace, size_t workspace_bytes,
                void* hip_stream) {
  return rib_forward_blend(h, B, H, W, label, img_fake, img_prev, img, mask, nullptr, workspace, workspace_bytes, hip_stream);
}

int rib_forward_blend(rib_handle* h, int B, int H, int W, const float* label, const float* img_fake,
                      const float* img_prev, float* img, float* mask, float* fuse, void* workspace, size_t workspace_bytes,
                      void* hip_stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!label || !img_fake || !img_prev || !img || !mask || !workspace) return fail(h, RIB_ERR_INVALID, "rib_forward: null pointer");
  Plan* P = get_plan(h, B, H, W);
  if (!P) return RIB_ERR_INVALID;
  if (workspace_bytes < P->ws_bytes) return fail(h, RIB_ERR_WORKSPACE, fmt("workspace %zu < required %zu bytes", workspace_bytes, P->ws_bytes));
  Resolver R; R.ws = reinterpret_cast<char*>(workspace); R.blob = h->d_blob; R.h = h;
  R.user[U_LABEL] = label; R.user[U_FAKE] = img_fake; R.user[U_PREV] = img_prev; R.user[U_IMG] = img; R.user[U_MASK] = mask;
  R.user[U_FUSE] = nullptr;
  bool fused = false;       // does the plan's mask head carry the blend?
  if (fuse)
    for (const Op& op : P->ops) fused = fused || op.fuse_blend;
  if (fused) R.user[U_FUSE] = fuse;
  rc = run_plan(h, P, R, reinterpret_cast<hipStream_t>(hip_stream));
  if (rc == RIB_OK && fuse && !fused) rc = rib_blend(h, B, h->g.c.image_nc, H, W, img, mask, img_fake, fuse, hip_stream);
  return rc;
}

namespace {
// label-only work is batched over the chain when it has more than one frame, on one stream (RIB_NO_LABEL_BATCH=1 disables)
static bool chain_batches_labels(const rib_handle* h, int T, int B) {
  // T * B * split-K (<= 16) indexes blockIdx.z (< 65536) of the batched launches
  return T > 1 && B < 128 && (long)T * B < 4096 && !getenv("RIB_NO_LABEL_BATCH");
}
}  // namespace

size_t rib_chain_workspace_bytes(rib_handle* h, int T, int B, int H, int W) {
  if (!h || T < 1) return 0;
  const size_t base = rib_workspace_bytes(h, B, H, W);
  if (base == 0 || !chain_batches_labels(h, T, B)) return base;
  Plan* PL = get_plan(h, T * B, H, W, PLAN_LABELS, B);
  return PL ? base + align256(PL->ws_bytes) : 0;
}

// (inside extern "C" an unnamed namespace does not keep a function's name out of the dynamic symbol table: static does)
static int chain_enqueue(rib_handle* h, int T, int B, int H, int W, const float* key_frame, const float* labels,
                         const float* dains, float* imgs, float* masks, float* fuses, void* workspace,
                         size_t workspace_bytes, void* hip_stream);

int rib_set_graph_replay(rib_handle* h, int enable) {
  if (!h) return RIB_ERR_INVALID;
  h->graph_replay = enable != 0;
  if (!h->graph_replay) drop_chain_graphs(h);
  return RIB_OK;
}

int rib_set_plan_batch(rib_handle* h, int n) {
  if (!h || n < 0) return RIB_ERR_INVALID;
  if (h->plan_batch != n) drop_chain_graphs(h);     // (plans are keyed by the batch they follow: nothing else to drop)
  h->plan_batch = n;
  return RIB_OK;
}

int rib_get_plan_batch(const rib_handle* h) { return h ? h->plan_batch : RIB_ERR_INVALID; }

int rib_graph_stats(rib_handle* h, int64_t* captures, int64_t* replays) {
  if (!h) return RIB_ERR_INVALID;
  if (captures) *captures = (int64_t)h->graph_captures;
  if (replays) *replays = (int64_t)h->graph_replays;
  return RIB_OK;
}

int rib_chain(rib_handle* h, int T, int B, int H, int W, const float* key_frame, const float* labels,
              const float* dains, float* imgs, float* masks, float* fuses, void* workspace,
              size_t workspace_bytes, void* hip_stream) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (T < 1 || !key_frame || !labels || !dains || !fuses || !workspace) return fail(h, RIB_ERR_INVALID, "rib_chain: bad argument");
  // (the NULL stream cannot be captured: a caller on it gets the launch-by-launch path)
  if (!h->graph_replay || h->profiling || h->device < 0 || hip_stream == nullptr)
    return chain_enqueue(h, T, B, H, W, key_frame, labels, dains, imgs, masks, fuses, workspace, workspace_bytes, hip_stream);
  // ---- graph replay: the T x ~130 launches of the segment as ONE graph launch.  Every kernel parameter is a function of the
  // shape and of the pointers of this call, so that tuple is the key; a call with other tensors captures its own graph (the
  // enqueue code runs under stream capture, nothing executes), at most 8 are kept.  Same kernels, same parameters, same order
  // on the same stream: the frames are bit-identical to the launch-by-launch path.
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const std::array<uintptr_t, 12> key = {(uintptr_t)T, (uintptr_t)B, (uintptr_t)H, (uintptr_t)W, (uintptr_t)key_frame, (uintptr_t)labels,
                                         (uintptr_t)dains, (uintptr_t)imgs, (uintptr_t)masks, (uintptr_t)fuses, (uintptr_t)workspace,
                                         (uintptr_t)workspace_bytes};
  for (auto& g : h->chain_graphs)
    if (g.key == key) {
      g.used = ++h->graph_clock; ++h->graph_replays; g.stream = st;
      HIP_TRY(h, hipGraphLaunch(g.exec, st));
      return RIB_OK;
    }
  // plans (and the Winograd filter sets they allocate) must exist before the capture starts: building one synchronises
  if (!get_plan(h, B, H, W, chain_batches_labels(h, T, B) ? PLAN_UNPAIRED : 0)) return RIB_ERR_INVALID;
  if (chain_batches_labels(h, T, B) && !get_plan(h, T * B, H, W, PLAN_LABELS, B)) return RIB_ERR_INVALID;
  hipGraph_t graph = nullptr;
  HIP_TRY(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  rc = chain_enqueue(h, T, B, H, W, key_frame, labels, dains, imgs, masks, fuses, workspace, workspace_bytes, hip_stream);
  const hipError_t ec = hipStreamEndCapture(st, &graph);
  if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (ec != hipSuccess) return fail(h, RIB_ERR_HIP, fmt("rib_chain: stream capture failed: %s", hipGetErrorString(ec)));
  hipGraphExec_t exec = nullptr;
  const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ei != hipSuccess) return fail(h, RIB_ERR_HIP, fmt("rib_chain: graph instantiation failed: %s", hipGetErrorString(ei)));
  if (h->chain_graphs.size() >= 8) {
    size_t lru = 0;
    for (size_t i = 1; i < h->chain_graphs.size(); ++i) if (h->chain_graphs[i].used < h->chain_graphs[lru].used) lru = i;
    destroy_chain_graph(h->chain_graphs[lru]);
    h->chain_graphs.erase(h->chain_graphs.begin() + lru);
  }
  h->chain_graphs.push_back({key, exec, ++h->graph_clock, st});
  ++h->graph_captures;
  HIP_TRY(h, hipGraphLaunch(exec, st));
  return RIB_OK;
}

static int chain_enqueue(rib_handle* h, int T, int B, int H, int W, const float* key_frame, const float* labels,
                         const float* dains, float* imgs, float* masks, float* fuses, void* workspace,
                         size_t workspace_bytes, void* hip_stream) {
  int rc = RIB_OK;
  // a chain that runs the label-only launches once per segment needs them apart from the image encoder's: the unpaired
  // twin of the frame plan (same kernels and choices: the frames equal rib_forward's bit for bit)
  Plan* P = get_plan(h, B, H, W, chain_batches_labels(h, T, B) ? PLAN_UNPAIRED : 0);
  if (!P) return RIB_ERR_INVALID;
  const rib_config& c = h->g.c;
  const size_t frame = (size_t)B * c.image_nc * H * W, mframe = (size_t)B * H * W, lframe = (size_t)B * c.label_nc * H * W;
  const size_t need = P->ws_bytes + 2 * align256(frame * sizeof(float)) + align256(mframe * sizeof(float));
  if (workspace_bytes < need) return fail(h, RIB_ERR_WORKSPACE, fmt("workspace %zu < required %zu bytes", workspace_bytes, need));
  char* wsb = reinterpret_cast<char*>(workspace);
  float* tmp_img = reinterpret_cast<float*>(wsb + P->ws_bytes);
  float* tmp_mask = reinterpret_cast<float*>(wsb + P->ws_bytes + align256(frame * sizeof(float)));
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  // The label maps of the whole segment are known up front: pack.label, down_first and the mask network's label
  // branch (8 + 9 launches, ~0.22 ms of a 3.0 ms frame at 512x512) run once at batch T*B, where the small maps fill
  // the chip, when the caller's workspace has room for it (rib_chain_workspace_bytes); each frame then copies its
  // slices into the frame plan's slots and skips those launches.
  Plan* PL = nullptr;
  char* lws = nullptr;
  if (chain_batches_labels(h, T, B)) {
    PL = get_plan(h, T * B, H, W, PLAN_LABELS, B);
    if (!PL) return RIB_ERR_INVALID;
    const size_t off = align256(need);
    if (workspace_bytes >= off + PL->ws_bytes) {
      lws = wsb + off;
      Resolver RL; RL.ws = lws; RL.blob = h->d_blob; RL.h = h;
      for (int u = 0; u < U_COUNT; ++u) RL.user[u] = nullptr;
      RL.user[U_LABEL] = labels;
      rc = run_plan(h, PL, RL, st);
      if (rc) return rc;
    } else PL = nullptr;     // a caller that sized the workspace with rib_workspace_bytes: per-frame label work
  }
  bool chain_fused = false;
  for (const Op& op : P->ops) chain_fused = chain_fused || op.fuse_blend;
  const float* prev = key_frame;   // evaluator.py:240-244: a segment starts from the ground-truth key frame
  for (int t = 0; t < T; ++t) {
    if (PL) {
      const LabelSlots& a = PL->ls; const LabelSlots& b = P->ls;   // a: [T*B] batch, b: [B] batch
      struct { size_t src, dst, bytes; } cp[6] = {{a.x0, b.x0, b.x0_b}, {a.nx_sc, b.nx_sc, b.nx_b}, {a.nx_sh, b.nx_sh, b.nx_b},
                                                   {a.cat, b.cat, b.cat_b}, {a.ncat_sc, b.ncat_sc, b.ncat_b}, {a.ncat_sh, b.ncat_sh, b.ncat_b}};
      Gather6Params gp;
      for (int k = 0; k < 6; ++k) {
        gp.src[k] = reinterpret_cast<const float4*>(lws + cp[k].src + (size_t)t * cp[k].bytes);
        gp.dst[k] = reinterpret_cast<float4*>(wsb + cp[k].dst);
        gp.n4[k] = (unsigned)(cp[k].bytes / 16);       // every slot is a whole number of 8-channel (32-byte) groups
      }
      RIB_KLAUNCH(k_gather6, dim3(1024, 6), dim3(256), 0, st, gp);
    }
    float* img_t = imgs ? imgs + (size_t)t * frame : tmp_img;
    float* mask_t = masks ? masks + (size_t)t * mframe : tmp_mask;
    float* fuse_t = fuses + (size_t)t * frame;
    Resolver R; R.ws = wsb; R.blob = h->d_blob; R.h = h;
    R.user[U_LABEL] = labels + (size_t)t * lframe; R.user[U_FAKE] = dains + (size_t)t * frame; R.user[U_PREV] = prev;
    R.user[U_IMG] = img_t; R.user[U_MASK] = mask_t;
    R.user[U_FUSE] = chain_fused ? fuse_t : nullptr;     // the mask head writes the blend itself when it can
    rc = run_plan(h, P, R, st, PL != nullptr);
    if (rc) return rc;
    if (!chain_fused) {
      rc = rib_blend(h, B, c.image_nc, H, W, img_t, mask_t, dains + (size_t)t * frame, fuse_t, hip_stream);
      if (rc) return rc;
    }
    prev = fuse_t;                 // evaluator.py:252: prev_img = results['fuse'][-1]
  }
  return RIB_OK;
}

int rib_set_debug_taps(rib_handle* h, int enable) {
  if (!h) return RIB_ERR_INVALID;
  if (h->keep_taps != (enable != 0)) { h->plans.clear(); drop_chain_graphs(h); }   // the workspace layout depends on it
  h->keep_taps = enable != 0;
  return RIB_OK;
}

int rib_set_wino_in_staging(rib_handle* h, int on) {
  if (!h) return RIB_ERR_INVALID;
  if (h->wino_in_staging != (on != 0)) { h->plans.clear(); drop_chain_graphs(h); }   // the grids of the .wino_in launches depend on it
  h->wino_in_staging = on != 0;
  return RIB_OK;
}

int rib_num_taps(rib_handle* h, int B, int H, int W) {
  if (!h) return RIB_ERR_INVALID;
  Plan* P = get_plan(h, B, H, W);
  return P ? (int)P->taps.size() : RIB_ERR_INVALID;
}

int rib_tap_info(rib_handle* h, int B, int H, int W, int idx, const char** name, int* C, int* th, int* tw) {
  if (!h) return RIB_ERR_INVALID;
  Plan* P = get_plan(h, B, H, W);
  if (!P || idx < 0 || idx >= (int)P->taps.size()) return RIB_ERR_INVALID;
  const Tap& t = P->taps[idx];
  if (name) *name = t.name.c_str();
  if (C) *C = t.C;
  if (th) *th = t.H;
  if (tw) *tw = t.W;
  return RIB_OK;
}

int rib_read_tap(rib_handle* h, int B, int H, int W, int idx, const void* workspace, float* dst, void* hip_stream) {
  if (!h || !workspace || !dst) return RIB_ERR_INVALID;
  if (!h->keep_taps) return fail(h, RIB_ERR_STATE, "rib_read_tap: call rib_set_debug_taps(h, 1) before the forward (intermediate buffers are reused otherwise)");
  Plan* P = get_plan(h, B, H, W);
  if (!P || idx < 0 || idx >= (int)P->taps.size()) return RIB_ERR_INVALID;
  const Tap& t = P->taps[idx];
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const float* src = reinterpret_cast<const float*>(reinterpret_cast<const char*>(workspace) + t.off);
  RIB_LAUNCH_ST(h->prec(), k_unpack, dim3((t.H * t.W + 255) / 256, B), dim3(256), 0, st, src, t.Cp, t.C, t.H * t.W, 0, t.H, t.W, dst);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(st));
  return RIB_OK;
}

// Inverse of the filter re-layout, from a host-only handle: used by the CPU tests to check the
// spectral-norm fold and the [CoutPad][tap][CinPad] / SPADE column layouts against the oracle.
int rib_debug_conv_weight(rib_handle* h, const char* conv_name, float* w_oihw, float* bias) {
  if (!h || !conv_name || !w_oihw || !bias) return RIB_ERR_INVALID;
  if (h->host_blob.empty()) return fail(h, RIB_ERR_STATE, "rib_debug_conv_weight needs a finalized host-only handle (device < 0)");
  auto it = h->conv_index.find(conv_name);
  if (it == h->conv_index.end() || !h->convs[it->second].used) return fail(h, RIB_ERR_INVALID, fmt("unknown conv '%s'", conv_name));
  const ConvDef& c = h->convs[it->second];
  const int taps = c.ks * c.ks;
  for (int o = 0; o < c.cout; ++o) {
    for (int i = 0; i < c.cin; ++i)
      for (int t = 0; t < taps; ++t)
        w_oihw[((size_t)o * c.cin + i) * taps + t] = h->host_blob[c.w_off + ((size_t)o * taps + t) * c.cinp + i];
    bias[o] = h->host_blob[c.b_off + o];
  }
  return RIB_OK;
}

int rib_debug_spade_weight(rib_handle* h, const char* conv_name, float* w_2c_by_cond, float* bias_2c) {
  if (!h || !conv_name || !w_2c_by_cond || !bias_2c) return RIB_ERR_INVALID;
  if (h->host_blob.empty()) return fail(h, RIB_ERR_STATE, "rib_debug_spade_weight needs a finalized host-only handle (device < 0)");
  const std::string cn = conv_name;
  const size_t pos = cn.rfind(".conv_block_");
  if (pos == std::string::npos) return fail(h, RIB_ERR_INVALID, "not a SPADE conv block");
  const std::string blk = cn.substr(0, pos), which = cn.substr(cn.size() - 1);
  const std::string key = blk + "." + (which == "s" ? std::string("0") : which);
  auto it = h->spade_index.find(key);
  if (it == h->spade_index.end()) return fail(h, RIB_ERR_INVALID, fmt("no SPADE group '%s'", key.c_str()));
  const SpadeGroup& sg = h->spades[it->second];
  const int set = which == "s" ? 1 : 0;
  const int condp = h->padc(sg.cond);
  for (int ch = 0; ch < sg.C; ++ch) {
    const int v = set * sg.Cp + ch;
    const int colg = (v / 32) * 64 + (v % 32), colb = colg + 32;
    for (int k = 0; k < sg.cond; ++k) {
      w_2c_by_cond[(size_t)ch * sg.cond + k] = h->host_blob[sg.w_off + (size_t)colg * condp + k];
      w_2c_by_cond[(size_t)(sg.C + ch) * sg.cond + k] = h->host_blob[sg.w_off + (size_t)colb * condp + k];
    }
    bias_2c[ch] = h->host_blob[sg.b_off + colg];
    bias_2c[sg.C + ch] = h->host_blob[sg.b_off + colb];
  }
  return RIB_OK;
}

// Launch list of a plan, for the CPU-side structure tests: "<name>|<kernel class>|<grid>|<tile>"
static int launch_info_head(const Op& op, char* buf, size_t buflen) {
  if (op.kind() == OP_IGEMM && op.small_co > 0)
    snprintf(buf, buflen, "%s|%d|%u,%u,%u|%s 16x16 tile, %d output channels%s|%.0f", op.name.c_str(), op.kclass, op.grid.x, op.grid.y, op.grid.z,
             op.head ? "head (taps as MFMA columns)" : "direct (vector ALUs)", op.small_co, op.fuse_blend ? " + fused blend" : "", op.flops);
  else if (op.kind() == OP_IGEMM)
    snprintf(buf, buflen, "%s|%d|%u,%u,%u|tile %dx%d BN %d BK %d s%d k%d ups%d ksplit%d kw%d tb%d%s v%d|%.0f", op.name.c_str(), op.kclass, op.grid.x, op.grid.y, op.grid.z,
             op.var->TH(), op.var->TW(), op.var->BN(), op.var->BK, op.var->STRIDE, op.var->KS, (int)op.var->UPS, op.as<IgemmParams>().ksplit, op.var->KW, op.var->DMAK ? 100 + (op.var->TB == 9 ? 9 : 0) : op.var->TB,
             op.wino ? (op.wino_m == 4 ? " wino4" : " wino") : "", (int)(op.var - kVariants), op.flops);      // (v<n>: index into rib_variant_info)
  else if (op.kind() == OP_GEMM)
    snprintf(buf, buflen, "%s|%d|%u,%u,%u|gemm (LDS-DMA staged operands) tile %dx%d BK 32, %d x [%d x %d x %d]%s|%.0f", op.name.c_str(), op.kclass, op.grid.x, op.grid.y, op.grid.z,
             op.var->BM(), op.var->BN(), (int)op.grid.z, op.as<GemmDmaParams>().M, op.as<GemmDmaParams>().N, op.as<GemmDmaParams>().K, (std::string(op.wino ? (op.wino_m == 4 ? " wino4" : " wino") : "") + (op.as<GemmDmaParams>().K2 ? fmt(" + K %d of the 1x1 shortcut at %d positions", op.as<GemmDmaParams>().K2, __builtin_popcountll(op.as<GemmDmaParams>().kmask)) : std::string())).c_str(), op.flops);
  else if (op.kind() == OP_LOWC)
    snprintf(buf, buflen, "%s|%d|%u,%u,%u|lowc (caller's NCHW tensors, K = 9 x %d real channels) 8x%d tile, %d columns|%.0f", op.name.c_str(), op.kclass,
             op.grid.x, op.grid.y, op.grid.z, op.lowc_ce, op.lowc_tw, op.lowc_ncol, op.flops);
  else if (op.kind() == OP_WINO_IN && op.wi_staged)
    snprintf(buf, buflen, "%s|%d|%u,%u,%u|staged, %dx%d tiles per workgroup|0", op.name.c_str(), op.kclass, op.grid.x, op.grid.y, op.grid.z,
             op.as<WinoInParams>().sty, op.as<WinoInParams>().stx);
  else
    snprintf(buf, buflen, "%s|%d|%u,%u,%u||0", op.name.c_str(), op.kclass, op.grid.x, op.grid.y, op.grid.z);
  return RIB_OK;
}

// Algorithmic HBM bytes of one launch (tools/prof_ops.py prices every launch against max(FLOPs / MFMA peak, these bytes / HBM)):
// every operand the launch NEEDS read once, every result written once - activations in the storage type, filters and
// statistics as stored; halo re-reads, split-K re-reads and L2 misses are exactly what this leaves out.  Whether a launch
// has an optional operand (residual, split-K slab, fused shortcut, join) is asked of its bindings: the pointer fields of the
// planned parameter structs are null until run_plan resolves its own copy.
static double op_algorithmic_bytes(const rib_handle* h, const Plan* P, const Op& op) {
  const double e = h->esz(), Bn = P->B;
  switch (op.kind()) {
    case OP_IGEMM: {
      const IgemmParams& p = op.as<IgemmParams>();
      const double samples = p.pair ? 2.0 * Bn : Bn;      // a paired launch carries two convolutions per image
      const int taps = op.var ? op.var->KS * op.var->KS : 9;
      double b = samples * p.Hin * p.Win * (double)p.Cin * e                         // input (or SPADE condition map)
                 + (double)p.CoutPad * taps * p.Cin * e * (p.pair ? 2.0 : 1.0)      // filters
                 + p.CoutPad * 4.0;                                                    // bias
      if (op.var && op.var->SPADE) {
        b += Bn * p.Hout * p.Wout * (double)p.C * e / (p.xm_ups ? 4.0 : 1.0);          // tensor being normalised
        b += Bn * p.Hout * p.Wout * (double)p.C * e * p.nsets;                         // modulated outputs
      } else if (op.bound(&IgemmParams::slab)) {
        b += (double)p.ksplit * samples * p.Hout * p.Wout * p.CoutPad * 4.0;           // split-K partial slabs (fp32)
      } else {
        b += samples * p.Hout * p.Wout * (double)p.Cout * (op.small_co > 0 || p.y_f32 ? 4.0 : e);
        if (op.bound(&IgemmParams::res)) b += samples * p.Hout * p.Wout * (double)p.Cout * e / (p.res_ups ? 4.0 : 1.0);
        if (op.bound(&IgemmParams::x2)) b += samples * p.Hout * p.Wout * (double)p.Cin2 * e + (double)p.CoutPad * p.Cin2 * e;
        // blend: img + dain read, fuse written (fp32 NCHW).  Whether it runs is known per call only (did the caller pass a
        // fused frame?); priced for every launch that can carry it
        if (op.fuse_blend) b += Bn * p.Hout * p.Wout * 3.0 * 4.0 * 3.0;
      }
      return b;
    }
    case OP_GEMM: {
      const GemmDmaParams& g = op.as<GemmDmaParams>();
      const double Z = op.grid.z;
      // (a fused shortcut: K2 more columns of both operands at the positions of kmask)
      const double z2 = g.K2 ? Bn * __builtin_popcountll(g.kmask) : 0.0, nb2 = g.K2 ? (double)__builtin_popcountll(g.kmask) : 0.0;
      return Z * g.M * (double)g.K * e + (g.modB ? (double)g.modB : 1.0) * g.N * (double)g.K * e + Z * g.M * (double)g.N * 4.0 +
             z2 * g.M * (double)g.K2 * e + nb2 * g.N * (double)g.K2 * e;
    }
    case OP_LOWC: {
      const LowcParams& l = op.as<LowcParams>();
      return Bn * l.H * l.W * (double)(l.c0 + l.c1 + l.c2) * 4.0 + Bn * l.H * l.W * (double)l.Cout * e + 9.0 * (l.c0 + l.c1 + l.c2) * l.Cout * 4.0;
    }
    case OP_POOL: { const PoolParams& q = op.as<PoolParams>(); return Bn * q.H * q.W * (double)q.C * e * 1.25; }
    case OP_INADD: { const InAddParams& q = op.as<InAddParams>(); return Bn * q.HW * (double)q.C * e * 3.0; }
    case OP_SPLITEPI: {
      const SplitEpiParams& q = op.as<SplitEpiParams>();
      return (double)q.ksplit * q.B * q.Hout * q.Wout * q.CoutPad * 4.0 + (double)q.B * q.Hout * q.Wout * q.Cout * e * (op.bound(&SplitEpiParams::res) ? 2.0 : 1.0);
    }
    case OP_MODULATE: {
      const ModulateParams& m = op.as<ModulateParams>();
      const double px = (double)m.B * m.Hout * m.Wout;
      return px * 2.0 * m.C * m.nsets * 4.0 * m.ksplit + px * m.C * e / (m.xm_ups ? 4.0 : 1.0) + px * m.C * e * m.nsets;
    }
    case OP_WINO_IN: {
      const WinoInParams& w = op.as<WinoInParams>();
      const int T = op.wino_m + 2;
      double b = Bn * w.H * w.W * (double)w.Cin * e / (w.x_ups ? 4.0 : 1.0) + Bn * w.tilesY * w.tilesX * (double)T * T * w.Cin * e;
      if (op.wi_mode != 0 && op.bound(&WinoInParams::slab)) b += Bn * w.H * w.W * 2.0 * w.Cin * 4.0;          // gamma/beta columns of the level slab
      if (op.wi_mode2 >= 0) {      // second source: read once (+ its gamma/beta columns when it is a lazy SPADE), V at m x m positions
        b += Bn * w.H * w.W * (double)w.Cin2 * e / (w.x2_ups ? 4.0 : 1.0) + Bn * w.tilesY * w.tilesX * (double)op.wino_m * op.wino_m * w.Cin2 * e;
        if (op.bound(&WinoInParams::slab2)) b += Bn * w.H * w.W * 2.0 * w.Cin2 * 4.0;
      } else
      if (op.bound(&WinoInParams::x2) || op.bound(&WinoInParams::xres)) b += Bn * w.H * w.W * (double)w.Cin * e * 2.0;               // join: second operand read, join stored
      return b;
    }
    case OP_WINO_OUT: {
      const WinoOutParams& w = op.as<WinoOutParams>();
      const int T = op.wino_m + 2;
      return Bn * w.tilesY * w.tilesX * (double)T * T * w.CoutPad * 4.0 + Bn * w.Hout * w.Wout * (double)w.Cout * e * (op.bound(&WinoOutParams::res) ? 2.0 : 1.0);
    }
    case OP_FINALIZE: { const FinalizeParams& q = op.as<FinalizeParams>(); return Bn * q.tiles * 2.0 * q.Cs * 8.0; }
    default: return 0.0;
  }
}

int rib_debug_launch_info(rib_handle* h, int B, int H, int W, int idx, char* buf, size_t buflen) {
  if (!h || !buf) return RIB_ERR_INVALID;
  Plan* P = get_plan(h, B, H, W);
  if (!P || idx < 0 || idx >= (int)P->ops.size()) return RIB_ERR_INVALID;
  const Op& op = P->ops[idx];
  const int rc = launch_info_head(op, buf, buflen);
  const size_t n = strlen(buf);
  if (n + 24 < buflen) snprintf(buf + n, buflen - n, "|%.0f", op_algorithmic_bytes(h, P, op));
  return rc;
}

// ---- tuning hooks: enumerate kernel variants, pin a (variant, split-K) choice for one op of one
// shape, and time a single op of the plan in isolation ----
const char* rib_build_info(void) {
  static const std::string info = [] {
#define RIB_X(s) rib_stamp_section_##s,
    const char* sh[RIB_NSECTIONS] = {RIB_FOR_SECTIONS(RIB_X)};
#undef RIB_X
    std::string s = std::string("librib stamp=") + (kLibStamp + sizeof("rib-stamp lib ") - 1) + " shards=";
    bool ok = true;
    for (int i = 0; i < RIB_NSECTIONS; ++i) {
      const char* hash = strrchr(sh[i], ' ');          // "rib-stamp shard<i> <hash>"
      hash = hash ? hash + 1 : "?";
      ok = ok && strcmp(hash, RIB_SHARD_STAMP) == 0;
      s += std::string(i ? "," : "") + hash;
    }
    ok = ok && strcmp(rib_frame_shared_stamp, RIB_SHARED_STAMP) == 0;      // both host objects saw the same rib::FrameState
    s += fmt(" consistent=%d variants=%d frame=%s compiler=%s", ok ? 1 : 0, kNumVariants, rib_stamp_frame + sizeof("rib-stamp frame ") - 1, __VERSION__);
    return s;
  }();
  return info.c_str();
}

int rib_num_variants(void) { return kNumVariants; }

int rib_variant_info(int idx, int geom[12]) {
  if (idx < 0 || idx >= kNumVariants || !geom) return RIB_ERR_INVALID;
  const Variant& v = kVariants[idx];
  const int g[12] = {v.FRW, v.WM, v.WN, v.MF, v.NF, v.BK, v.STRIDE, v.KS, v.UPS ? 1 : 0, v.SPADE ? 1 : 0, v.KW, v.DMAK ? 100 + (v.TB == 9 ? 9 : 0) : v.TB};
  for (int i = 0; i < 12; ++i) geom[i] = g[i];
  return v.BF16;   // precision of the instantiation: 0 fp32, 1 bf16 storage, 2 half storage
}

int rib_set_choice(rib_handle* h, int B, int H, int W, const char* op_name, int variant_idx, int ksplit) {
  if (!h || !op_name) return RIB_ERR_INVALID;
  const std::string key = fmt("%d,%d,%d|%s", B, H, W, op_name);
  if (variant_idx < 0) h->choices.erase(key);
  else {
    if (variant_idx >= kNumVariants || ksplit < 1) return fail(h, RIB_ERR_INVALID, "rib_set_choice: bad variant / ksplit");
    h->choices[key] = {variant_idx, ksplit};
  }
  drop_chain_graphs(h);
  // the frame plans of this shape (paired and unpaired) are rebuilt on next use, and so are the labels-only plans of
  // chains that follow this shape's choices (key {flags, tuneB, batch, H, W})
  for (auto it = h->plans.begin(); it != h->plans.end();) {
    const std::array<int, 5>& k = it->first;
    const bool same_hw = k[3] == H && k[4] == W;
    const bool follows = same_hw && (k[1] > 0 ? k[1] : k[2]) == B;      // the batch whose choices the plan follows
    if (follows) it = h->plans.erase(it); else ++it;
  }
  return RIB_OK;
}

int rib_time_op(rib_handle* h, int B, int H, int W, const char* op_name, const float* label, const float* img_fake,
                const float* img_prev, float* img, float* mask, void* workspace, size_t workspace_bytes, int iters,
                void* hip_stream, double* usec) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!op_name || !workspace || !usec || iters < 1) return RIB_ERR_INVALID;
  Plan* P = get_plan(h, B, H, W);
  if (!P) return RIB_ERR_INVALID;
  if (workspace_bytes < P->ws_bytes) return fail(h, RIB_ERR_WORKSPACE, "rib_time_op: workspace too small");
  // a sub-plan holding the op and, for split-K, its slab-summing epilogue
  Plan sub; sub.B = B; sub.H = H; sub.W = W;
  const std::string nm = op_name;
  for (const Op& op : P->ops)
    if (op.name == nm || op.name == nm + ".splitk_sum" || op.name == nm + ".modulate" || op.for_op == nm) sub.ops.push_back(op);
  if (sub.ops.empty()) return fail(h, RIB_ERR_INVALID, fmt("rib_time_op: no op named '%s'", op_name));
  Resolver R; R.ws = reinterpret_cast<char*>(workspace); R.blob = h->d_blob; R.h = h;
  R.user[U_LABEL] = label; R.user[U_FAKE] = img_fake; R.user[U_PREV] = img_prev; R.user[U_IMG] = img; R.user[U_MASK] = mask;
  R.user[U_FUSE] = nullptr;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  const bool was = h->profiling; h->profiling = false;
  rc = run_plan(h, &sub, R, st);   // warm-up
  hipEvent_t e0, e1;
  HIP_TRY(h, hipEventCreate(&e0)); HIP_TRY(h, hipEventCreate(&e1));
  HIP_TRY(h, hipEventRecord(e0, st));
  for (int i = 0; i < iters && rc == RIB_OK; ++i) rc = run_plan(h, &sub, R, st);
  HIP_TRY(h, hipEventRecord(e1, st));
  HIP_TRY(h, hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(h, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  h->profiling = was;
  *usec = (double)ms * 1e3 / iters;
  return rc;
}

static void drop_prof_events(rib_handle* h) {
  for (auto& pe : h->prof_events) (void)hipEventDestroy(pe.second);
  h->prof_events.clear();
  for (auto& ke : h->prof_kernel_events) { (void)hipEventDestroy(ke.start); (void)hipEventDestroy(ke.stop); }
  h->prof_kernel_events.clear();
}

int rib_profile_begin(rib_handle* h) {
  if (!h) return RIB_ERR_INVALID;
  drop_prof_events(h);
  h->profiling = true; h->prof_kernels = false;
  return RIB_OK;
}

int rib_profile_begin_kernels(rib_handle* h) {
  if (!h) return RIB_ERR_INVALID;
  drop_prof_events(h);
  h->profiling = true; h->prof_kernels = true;
  return RIB_OK;
}

int rib_profile_collect(rib_handle* h, int64_t launches[RIB_KC_COUNT], double ms[RIB_KC_COUNT]) {
  if (!h || !launches || !ms) return RIB_ERR_INVALID;
  h->profiling = false;
  for (int i = 0; i < RIB_KC_COUNT; ++i) { launches[i] = 0; ms[i] = 0.0; }
  if (h->prof_kernels) {
    if (!h->prof_kernel_events.empty()) HIP_TRY(h, hipEventSynchronize(h->prof_kernel_events.back().stop));
    for (const auto& ke : h->prof_kernel_events) {
      float t = 0.f;
      HIP_TRY(h, hipEventElapsedTime(&t, ke.start, ke.stop));
      launches[ke.kclass] += 1; ms[ke.kclass] += (double)t;
    }
    drop_prof_events(h);
    h->prof_kernels = false;
    return RIB_OK;
  }
  if (!h->prof_events.empty()) HIP_TRY(h, hipEventSynchronize(h->prof_events.back().second));
  for (size_t i = 0; i + 1 < h->prof_events.size(); ++i) {
    const int kc = h->prof_events[i].first;
    if (kc < 0) continue;                       // end marker of a plan run: the gap to the next run belongs to no launch
    float t = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&t, h->prof_events[i].second, h->prof_events[i + 1].second));
    launches[kc] += 1; ms[kc] += (double)t;
  }
  drop_prof_events(h);
  return RIB_OK;
}

int rib_forward_flops(rib_handle* h, int B, int H, int W, double flops[RIB_KC_COUNT]) {
  if (!h || !flops) return RIB_ERR_INVALID;
  Plan* P = get_plan(h, B, H, W);
  if (!P) return RIB_ERR_INVALID;
  for (int i = 0; i < RIB_KC_COUNT; ++i) flops[i] = P->flops[i];
  return RIB_OK;
}

int rib_num_launches(rib_handle* h, int B, int H, int W) {
  if (!h) return RIB_ERR_INVALID;
  Plan* P = get_plan(h, B, H, W);
  return P ? (int)P->ops.size() : RIB_ERR_INVALID;
}

}  // extern "C"
