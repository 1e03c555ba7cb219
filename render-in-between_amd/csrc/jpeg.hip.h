// jpeg.hip.h — baseline JPEG of the folder driver's diagnostic sheets, encoded on the GPU (rib_jpeg, include/rib.h).
//
// panel.py (jpeg_encode_host) states the file as an exact integer definition - baseline sequential DCT, 8 bit, Y Cb Cr 4:2:0,
// the Annex K tables of ITU-T T.81 under the IJG quality scaling, a restart interval of one MCU row - and these kernels write
// the same bytes from the uint8 HWC sheets that rib_panel left on the device, so that ~1/20 of a sheet's bytes travel home and
// no host core encodes it.  Every number below is panel.py's; the arithmetic is restated there line by line.
//
//   k_jpeg_segments  grid (MCU rows, T), 256 threads: a workgroup owns ONE restart segment (one MCU row of one frame) and walks
//                    it in chunks of JPEG_CHUNK MCUs (96 blocks, 256 pixels wide):
//                      1. the chunk's 16 sheet rows come in as aligned dwords into LDS (byte loads only where a dword would
//                         reach outside the source tensor); the float instantiation (rib_jpeg_float: frames fp32 NCHW in [-1, 1])
//                         reads four pixels of the three channel planes per thread instead - float4 where the plane's row
//                         segment is 16-byte aligned and whole, scalar loads otherwise - quantises them (quantise_u8: the
//                         arithmetic of k_quantise) and stores the same interleaved RGB bytes, at phase 0;
//                      2. a thread per 2 x 2 pixels: fixed-point Y Cb Cr, chroma as the rounded mean, level shift, int16
//                         samples block by block in LDS (edge MCUs read the last column / row again);
//                      3. the DCT row pass, a thread per block row, in place; the column pass, a thread per block column, into
//                         registers, quantised, then written in zig-zag order (int32 throughout, bounds in panel.py);
//                      4. a thread per block: the bits its symbols take; every thread sums the lengths in front of it;
//                      5. a thread per block: its symbols again, packed most significant bit first into a zeroed LDS bit
//                         buffer (integer OR on LDS words: deterministic);
//                      6. whole bytes leave for the segment's staging slot, 0xFF followed by 0x00 (a ballot scan per 256
//                         bytes); the unfinished last byte and the three DC predictors carry into the next chunk; the last
//                         chunk is filled with 1-bits first.
//                    The slot is jpeg_seg_bound(cols) bytes (bound below): never exceeded, and still checked on every store.
//   k_jpeg_assemble  grid (MCU rows, T), 256 threads: a workgroup sums the segment lengths of its frame in front of its own
//                    (and all of them: the file length), then copies its segment behind the header and the earlier ones,
//                    RSTn in front of it; row 0 also writes the header and lengths[t], the last row EOI.  A frame that does
//                    not fit dst_stride writes nothing and gets length 0.
//
// Staging bound: a block emits at most 64 symbols (one DC, 63 AC) of at most 16 + 11 bits (the true worst case, 20 + 63 * 26
// bits, is smaller: a ZRL or an EOB stands for coefficients that would each cost more), i.e. 216 bytes; a segment of
// n = 6 * cols blocks is at most 216 n bytes before stuffing and twice that when every byte is 0xFF.
// No atomics on global memory, no floats behind step 1, nothing depends on T or on the order in which workgroups run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "pixel_ops.hip.h"

namespace rib {

constexpr int JPEG_HEADER_BYTES = 629;                  // panel.JPEG_HEADER_BYTES
constexpr int JPEG_CHUNK = 16;                          // MCUs per chunk: 96 blocks, 256 pixels
constexpr int JPEG_BLOCKS = JPEG_CHUNK * 6;
constexpr int JPEG_BLOCK_STRIDE = 66;                   // int16 per block in LDS: 33 dwords, a thread per block hits 64 different banks
constexpr int JPEG_RAW_STRIDE = 776;                    // bytes per sheet row of a chunk in LDS: up to 3 of phase + 768 + 3 of tail, 194 dwords
constexpr int JPEG_A_WORDS = JPEG_BLOCKS * 216 / 4 + 4; // the bit buffer (a chunk at its bound, the carried byte, slack); >= 16 * 776 / 4
constexpr int JPEG_MAX_DIM = 65535;
inline size_t jpeg_seg_bound(int cols) { return (size_t)2 * 216 * 6 * (size_t)cols; }

#define RIB_JPEG_QLUM {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62, \
  18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99}
#define RIB_JPEG_QCHR {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}
#define RIB_JPEG_ZIGZAG {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, \
  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
#define RIB_JPEG_DC_BITS {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}}
#define RIB_JPEG_AC_BITS {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}}
#define RIB_JPEG_AC_VALS {{1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, \
  36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, \
  88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, \
  150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, \
  201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250}, \
  {0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, \
  36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, \
  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, \
  152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, \
  210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}}

// the tables twice: for the kernels, and for the host that writes the header
__constant__ uint8_t c_jpeg_qbase[2][64] = {RIB_JPEG_QLUM, RIB_JPEG_QCHR};
__constant__ uint8_t c_jpeg_zigzag[64] = RIB_JPEG_ZIGZAG;
__constant__ uint8_t c_jpeg_dc_bits[2][16] = RIB_JPEG_DC_BITS;
__constant__ uint8_t c_jpeg_ac_bits[2][16] = RIB_JPEG_AC_BITS;
__constant__ uint8_t c_jpeg_ac_vals[2][162] = RIB_JPEG_AC_VALS;
static const uint8_t h_jpeg_qbase[2][64] = {RIB_JPEG_QLUM, RIB_JPEG_QCHR};
static const uint8_t h_jpeg_zigzag[64] = RIB_JPEG_ZIGZAG;
static const uint8_t h_jpeg_dc_bits[2][16] = RIB_JPEG_DC_BITS;
static const uint8_t h_jpeg_ac_bits[2][16] = RIB_JPEG_AC_BITS;
static const uint8_t h_jpeg_ac_vals[2][162] = RIB_JPEG_AC_VALS;

// IJG quality scaling of one base entry (panel.jpeg_qtables)
__host__ __device__ inline int jpeg_qscale(int base, int quality) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (base * scale + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}

struct JpegHeader { uint8_t b[JPEG_HEADER_BYTES + 3]; };

// panel.jpeg_header, byte for byte
inline void jpeg_make_header(JpegHeader& hd, int H, int W, int quality) {
  uint8_t* p = hd.b;
  auto put = [&](std::initializer_list<int> v) { for (int x : v) *p++ = (uint8_t)x; };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int c = 0; c < 2; ++c) {
    put({0xFF, 0xDB, 0, 67, c});
    for (int k = 0; k < 64; ++k) *p++ = (uint8_t)jpeg_qscale(h_jpeg_qbase[c][h_jpeg_zigzag[k]], quality);
  }
  put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int c = 0; c < 2; ++c) {
    put({0xFF, 0xC4, 0, 19 + 12, c});
    for (int k = 0; k < 16; ++k) *p++ = h_jpeg_dc_bits[c][k];
    for (int k = 0; k < 12; ++k) *p++ = (uint8_t)k;
    put({0xFF, 0xC4, 0, 19 + 162, 0x10 | c});
    for (int k = 0; k < 16; ++k) *p++ = h_jpeg_ac_bits[c][k];
    for (int k = 0; k < 162; ++k) *p++ = h_jpeg_ac_vals[c][k];
  }
  const int cols = (W + 15) / 16;
  put({0xFF, 0xDD, 0, 4, cols >> 8, cols & 255});
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

template <typename S>
struct JpegParamsT {
  const S* src;             // uint8_t: [T, H, W, 3]; float: [T, 3, H, W] in [-1, 1]
  uint8_t* seg;             // [T, rows] slots of `slot` bytes
  int32_t* seglen;          // [T, rows]: bytes of the segment, -1: the slot would have been exceeded
  int H, W, quality, rows, cols;
  uint32_t slot;
};
using JpegParams = JpegParamsT<uint8_t>;

// one pass of the 8-point DCT in 13 fractional bits: o[u] = (sum_x K[u][x] s[x] + rnd) >> sh (panel._JPEG_DCT)
__device__ inline void jpeg_dct8(const int s[8], int o[8], int rnd, int sh) {
  constexpr int K[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},   {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                           {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                           {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                           {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int acc = rnd;
#pragma unroll
    for (int x = 0; x < 8; ++x) acc += K[u][x] * s[x];
    o[u] = acc >> sh;
  }
}

__device__ inline int jpeg_category(int v) { return 32 - __clz(v < 0 ? -v : v); }      // bits of |v|; 0 for 0

// the DC predictor of block b of a chunk: the component's previous block, or what the last chunk left
__device__ inline int jpeg_dc_pred(const int16_t* coef, const int* pred, int b) {
  const int m = b / 6, j = b - m * 6;
  if (j >= 1 && j <= 3) return coef[(b - 1) * JPEG_BLOCK_STRIDE];
  if (m == 0) return pred[j < 4 ? 0 : j - 3];
  return coef[((m - 1) * 6 + (j == 0 ? 3 : j)) * JPEG_BLOCK_STRIDE];
}

// a bit writer of one thread into the chunk's zeroed LDS bit buffer, most significant bit first; words are shared with the
// neighbouring blocks at both ends, hence the integer OR
struct JpegBits {
  uint32_t* words;
  uint64_t acc;
  int n, wi;
  __device__ void start(uint32_t* w, int bitpos) { words = w; acc = 0; n = bitpos & 31; wi = bitpos >> 5; }
  __device__ void put(uint32_t code, int len) {          // len <= 27, n < 32
    if (len == 0) return;
    acc |= (uint64_t)code << (64 - n - len);
    n += len;
    if (n >= 32) {
      atomicOr(&words[wi], __builtin_bswap32((uint32_t)(acc >> 32)));
      ++wi;
      acc <<= 32;
      n -= 32;
    }
  }
  __device__ void finish() { if (n > 0) atomicOr(&words[wi], __builtin_bswap32((uint32_t)(acc >> 32))); }
};

// four pixels of one channel plane's row as bytes 0..3 (float source): `valid` of them exist
__device__ inline uint32_t jpeg_quantise4(const float* a, int valid) {
  if (valid >= 4 && (reinterpret_cast<uintptr_t>(a) & 15) == 0) {
    const float4 v = *reinterpret_cast<const float4*>(a);
    return (uint32_t)quantise_u8(v.x) | ((uint32_t)quantise_u8(v.y) << 8) | ((uint32_t)quantise_u8(v.z) << 16) | ((uint32_t)quantise_u8(v.w) << 24);
  }
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < valid) r |= (uint32_t)quantise_u8(a[k]) << (8 * k);
  return r;
}

template <typename S>
__global__ __launch_bounds__(256) void k_jpeg_segments(JpegParamsT<S> p) {
  constexpr bool kU8 = std::is_same<S, uint8_t>::value;
  __shared__ __attribute__((aligned(16))) uint32_t s_a[JPEG_A_WORDS];            // the chunk's raw rows, later its bit buffer
  __shared__ __attribute__((aligned(16))) int16_t s_coef[JPEG_BLOCKS * JPEG_BLOCK_STRIDE];
  __shared__ uint32_t s_ac[2][256];        // code << 8 | length by symbol
  __shared__ uint32_t s_dc[2][16];
  __shared__ uint16_t s_q[2][64];          // natural order
  __shared__ uint8_t s_izz[64];            // natural position -> zig-zag index
  __shared__ int s_len[JPEG_BLOCKS];
  __shared__ int s_pred[3];
  __shared__ int s_wsum[4];
  __shared__ uint32_t s_carry;
  const int tid = threadIdx.x, row = blockIdx.x, t = blockIdx.y;
  const int H = p.H, W = p.W;
  uint8_t* const s_raw = reinterpret_cast<uint8_t*>(s_a);

  // ---- tables ----
  for (int i = tid; i < 512; i += 256) (&s_ac[0][0])[i] = 0;
  if (tid < 32) (&s_dc[0][0])[tid] = 0;
  if (tid < 128) s_q[tid >> 6][tid & 63] = (uint16_t)jpeg_qscale(c_jpeg_qbase[tid >> 6][tid & 63], p.quality);
  if (tid < 64) s_izz[c_jpeg_zigzag[tid]] = (uint8_t)tid;
  if (tid < 3) s_pred[tid] = 0;
  __syncthreads();
  for (int i = tid; i < 2 * 256; i += 256) {             // Annex C: the k-th symbol's code, from the counts per length
    const int c = i >> 8, k = i & 255;
    const bool dc = k >= 162;                            // 162 AC symbols, then the 12 DC symbols
    const int kk = dc ? k - 162 : k;
    if (dc && kk >= 12) continue;
    const uint8_t* bits = dc ? c_jpeg_dc_bits[c] : c_jpeg_ac_bits[c];
    int code = 0, base = 0;
    for (int l = 1; l <= 16; ++l) {
      const int n = bits[l - 1];
      if (kk < base + n) {
        const uint32_t e = ((uint32_t)(code + kk - base) << 8) | (uint32_t)l;
        if (dc) s_dc[c][kk] = e; else s_ac[c][c_jpeg_ac_vals[c][kk]] = e;
        break;
      }
      code = (code + n) << 1;
      base += n;
    }
  }
  __syncthreads();

  const int y0 = row * 16;
  const int nrows = min(16, H - y0);                     // sheet rows this MCU row really has
  const uint8_t* src_lo = nullptr;
  const uint8_t* src_hi = nullptr;
  if constexpr (kU8) {
    src_lo = p.src;
    src_hi = p.src + (size_t)gridDim.y * H * W * 3;
  }
  uint8_t* const out = p.seg + ((size_t)t * p.rows + row) * p.slot;
  uint32_t outpos = 0;                                   // bytes of the segment so far (uniform)
  int carrybits = 0;                                     // bits of the unfinished byte carried into this chunk (uniform)

  for (int m0 = 0; m0 < p.cols; m0 += JPEG_CHUNK) {
    const int ncm = min(JPEG_CHUNK, p.cols - m0);
    const int nblk = ncm * 6;
    const int x0 = m0 * 16;
    const int npx = min(ncm * 16, W - x0);               // sheet columns this chunk really has
    // ---- 1. the chunk's rows -> LDS, at their own phase inside a dword ----
    const uint8_t* g0 = nullptr;                         // uint8 source: the chunk's first byte
    if constexpr (kU8) {
    g0 = p.src + (((size_t)t * H + y0) * W + x0) * 3;
    for (int ry = 0; ry < nrows; ++ry) {
      const uint8_t* g = g0 + (size_t)ry * W * 3;
      const int phase = (int)(reinterpret_cast<uintptr_t>(g) & 3);
      const int ndw = (phase + npx * 3 + 3) >> 2;        // <= 193
      for (int j = tid; j < ndw; j += 256) {
        const uint8_t* a = g - phase + 4 * j;
        uint32_t v;
        if (a >= src_lo && a + 4 <= src_hi) {
          v = *reinterpret_cast<const uint32_t*>(a);
        } else {
          v = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (a + k >= src_lo && a + k < src_hi) v |= (uint32_t)a[k] << (8 * k);
        }
        s_a[(ry * JPEG_RAW_STRIDE >> 2) + j] = v;
      }
    }
    } else {
      // float source: a thread takes four pixels of a row from each of the three planes (12 bytes, three dwords of the row)
      const int nq4 = (npx + 3) >> 2;                    // <= 64
      const size_t plane = (size_t)H * W;
      const float* f0 = p.src + (size_t)t * 3 * plane + (size_t)y0 * W + x0;
      for (int task = tid; task < nrows * nq4; task += 256) {
        const int ry = task / nq4, j = task - ry * nq4;
        const float* a = f0 + (size_t)ry * W + 4 * j;
        const int valid = npx - 4 * j;                   // >= 1: pixels of this row from 4 j on
        const uint32_t r = jpeg_quantise4(a, valid), g = jpeg_quantise4(a + plane, valid), b = jpeg_quantise4(a + 2 * plane, valid);
        uint32_t* d = s_a + (ry * JPEG_RAW_STRIDE >> 2) + 3 * j;      // bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        d[0] = (r & 0xFFu) | ((g & 0xFFu) << 8) | ((b & 0xFFu) << 16) | ((r & 0xFF00u) << 16);
        d[1] = ((g >> 8) & 0xFFu) | (b & 0xFF00u) | (r & 0xFF0000u) | ((g & 0xFF0000u) << 8);
        d[2] = ((b >> 16) & 0xFFu) | ((r >> 16) & 0xFF00u) | ((g >> 8) & 0xFF0000u) | (b & 0xFF000000u);
      }
    }
    __syncthreads();
    // ---- 2. colour, chroma mean, level shift ----
    for (int q = tid; q < ncm * 8 * 8; q += 256) {       // 2 x 2 pixels each: 8 quad rows, 8 quad columns per MCU
      const int qy = q / (ncm * 8), qx = q - qy * (ncm * 8);
      int cbs = 2, crs = 2;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const int py = qy * 2 + dy;
        const int ry = min(py, nrows - 1);
        int phase = 0;                                   // the float source's bytes start the LDS row
        if constexpr (kU8) phase = (int)(reinterpret_cast<uintptr_t>(g0 + (size_t)ry * W * 3) & 3);
        const uint8_t* lrow = s_raw + ry * JPEG_RAW_STRIDE + phase;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int px = qx * 2 + dx;
          const uint8_t* c = lrow + min(px, npx - 1) * 3;
          const int r = c[0], gg = c[1], b = c[2];
          const int y = (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
          cbs += (-11059 * r - 21709 * gg + 32768 * b + 8421375) >> 16;
          crs += (32768 * r - 27439 * gg - 5329 * b + 8421375) >> 16;
          const int blk = (px >> 4) * 6 + ((py >> 3) << 1) + ((px >> 3) & 1);
          s_coef[blk * JPEG_BLOCK_STRIDE + (py & 7) * 8 + (px & 7)] = (int16_t)(y - 128);
        }
      }
      const int cb = (qx >> 3) * 6 + 4;
      s_coef[cb * JPEG_BLOCK_STRIDE + qy * 8 + (qx & 7)] = (int16_t)((cbs >> 2) - 128);
      s_coef[(cb + 1) * JPEG_BLOCK_STRIDE + qy * 8 + (qx & 7)] = (int16_t)((crs >> 2) - 128);
    }
    __syncthreads();
    // ---- 3. DCT: rows in place, columns through registers into zig-zag order, quantised ----
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int task = tid + 256 * i, b = task >> 3, y = task & 7;
      if (b < nblk) {
        int16_t* v = s_coef + b * JPEG_BLOCK_STRIDE + y * 8;
        int s[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) s[x] = v[x];
        jpeg_dct8(s, o, 512, 10);
#pragma unroll
        for (int x = 0; x < 8; ++x) v[x] = (int16_t)o[x];
      }
    }
    __syncthreads();
    int16_t qv[3][8];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int task = tid + 256 * i, b = task >> 3, u = task & 7;
      if (b < nblk) {
        const int16_t* v = s_coef + b * JPEG_BLOCK_STRIDE + u;
        const int tab = (b % 6) >= 4 ? 1 : 0;
        int s[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) s[y] = v[y * 8];
        jpeg_dct8(s, o, 32768, 16);
#pragma unroll
        for (int y = 0; y < 8; ++y) {
          const int Q = s_q[tab][y * 8 + u];
          const int a = ((o[y] < 0 ? -o[y] : o[y]) + (Q >> 1)) / Q;
          qv[i][y] = (int16_t)(o[y] < 0 ? -a : a);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int task = tid + 256 * i, b = task >> 3, u = task & 7;
      if (b < nblk) {
#pragma unroll
        for (int y = 0; y < 8; ++y) s_coef[b * JPEG_BLOCK_STRIDE + s_izz[y * 8 + u]] = qv[i][y];
      }
    }
    __syncthreads();
    // ---- 4. bits per block ----
    if (tid < nblk) {
      const int16_t* v = s_coef + tid * JPEG_BLOCK_STRIDE;
      const int tab = (tid % 6) >= 4 ? 1 : 0;
      const int cat = jpeg_category(v[0] - jpeg_dc_pred(s_coef, s_pred, tid));
      int bits = (int)(s_dc[tab][cat] & 255) + cat;
      const int zrl = (int)(s_ac[tab][0xF0] & 255);
      int run = 0;
      for (int k = 1; k < 64; ++k) {
        const int c = v[k];
        if (c == 0) { ++run; continue; }
        const int n = jpeg_category(c);
        bits += (run >> 4) * zrl + (int)(s_ac[tab][((run & 15) << 4) | n] & 255) + n;
        run = 0;
      }
      if (run) bits += (int)(s_ac[tab][0] & 255);
      s_len[tid] = bits;
    }
    __syncthreads();
    int before = carrybits, total = carrybits;
    for (int b = 0; b < nblk; ++b) {
      const int l = s_len[b];
      total += l;
      if (b < tid) before += l;
    }
    const bool last = m0 + JPEG_CHUNK >= p.cols;
    const int nwords = min(JPEG_A_WORDS, ((total + 31) >> 5) + 1);
    for (int i = tid; i < nwords; i += 256) s_a[i] = i == 0 ? s_carry & (carrybits ? 0xFFu : 0u) : 0u;
    __syncthreads();
    // ---- 5. the symbols ----
    if (tid < nblk) {
      const int16_t* v = s_coef + tid * JPEG_BLOCK_STRIDE;
      const int tab = (tid % 6) >= 4 ? 1 : 0;
      JpegBits w;
      w.start(s_a, before);
      const int diff = v[0] - jpeg_dc_pred(s_coef, s_pred, tid);
      const int cat = jpeg_category(diff);
      w.put(s_dc[tab][cat] >> 8, (int)(s_dc[tab][cat] & 255));
      w.put((uint32_t)(diff < 0 ? diff + (1 << cat) - 1 : diff), cat);
      const uint32_t zrl = s_ac[tab][0xF0];
      int run = 0;
      for (int k = 1; k < 64; ++k) {
        const int c = v[k];
        if (c == 0) { ++run; continue; }
        for (; run > 15; run -= 16) w.put(zrl >> 8, (int)(zrl & 255));
        const int n = jpeg_category(c);
        const uint32_t e = s_ac[tab][(run << 4) | n];
        const int hl = (int)(e & 255);
        w.put(((e >> 8) << n) | (uint32_t)(c < 0 ? c + (1 << n) - 1 : c), hl + n);      // <= 16 + 10 bits
        run = 0;
      }
      if (run) w.put(s_ac[tab][0] >> 8, (int)(s_ac[tab][0] & 255));
      w.finish();
    }
    __syncthreads();
    // ---- 6. whole bytes leave, stuffed; the rest carries ----
    int nfull = total >> 3;
    const int rem = total & 7;
    if (tid == 0) {
      s_pred[0] = s_coef[((ncm - 1) * 6 + 3) * JPEG_BLOCK_STRIDE];
      s_pred[1] = s_coef[((ncm - 1) * 6 + 4) * JPEG_BLOCK_STRIDE];
      s_pred[2] = s_coef[((ncm - 1) * 6 + 5) * JPEG_BLOCK_STRIDE];
      if (last && rem) s_raw[nfull] |= (uint8_t)((1 << (8 - rem)) - 1);                 // the segment ends on a byte: 1-bits
      s_carry = s_raw[nfull];
    }
    __syncthreads();
    if (last && rem) ++nfull;
    carrybits = last ? 0 : rem;
    for (int i0 = 0; i0 < nfull; i0 += 256) {
      const int i = i0 + tid;
      const uint32_t byte = i < nfull ? s_raw[i] : 0u;
      const bool ff = byte == 0xFFu;
      const unsigned long long mask = __ballot(ff);
      const int lane = tid & 63, wave = tid >> 6;
      if (lane == 0) s_wsum[wave] = __popcll(mask);
      __syncthreads();
      int pre = __popcll(mask & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) pre += s_wsum[w];
        all += s_wsum[w];
      }
      const uint32_t pos = outpos + (uint32_t)(i - i0 + pre);
      if (i < nfull) {
        if (pos < p.slot) out[pos] = (uint8_t)byte;
        if (ff && pos + 1 < p.slot) out[pos + 1] = 0;
      }
      outpos += (uint32_t)(min(256, nfull - i0) + all);
      __syncthreads();
    }
  }
  if (tid == 0) p.seglen[(size_t)t * p.rows + row] = outpos <= p.slot ? (int32_t)outpos : -1;
}

struct JpegAssembleParams {
  const uint8_t* seg;
  const int32_t* seglen;
  uint8_t* dst;
  int32_t* lengths;
  size_t dst_stride;
  int rows;
  uint32_t slot;
  JpegHeader header;
};

__global__ __launch_bounds__(256) void k_jpeg_assemble(JpegAssembleParams p) {
  __shared__ unsigned long long s_sum[2][256];
  __shared__ int s_bad[256];
  const int tid = threadIdx.x, row = blockIdx.x, t = blockIdx.y;
  const int32_t* len = p.seglen + (size_t)t * p.rows;
  unsigned long long before = 0, all = 0;
  int bad = 0;
  for (int r = tid; r < p.rows; r += 256) {
    const int32_t l = len[r];
    if (l < 0) { bad = 1; continue; }
    all += (unsigned long long)l;
    if (r < row) before += (unsigned long long)l;
  }
  s_sum[0][tid] = before; s_sum[1][tid] = all; s_bad[tid] = bad;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {                    // integer sums: the order does not matter
    if (tid < s) { s_sum[0][tid] += s_sum[0][tid + s]; s_sum[1][tid] += s_sum[1][tid + s]; s_bad[tid] |= s_bad[tid + s]; }
    __syncthreads();
  }
  const unsigned long long total = (unsigned long long)JPEG_HEADER_BYTES + s_sum[1][0] + 2ull * (unsigned long long)(p.rows - 1) + 2ull;
  const bool refused = s_bad[0] || total > (unsigned long long)p.dst_stride;
  if (row == 0 && tid == 0) p.lengths[t] = refused ? 0 : (int32_t)total;
  if (refused) return;
  uint8_t* f = p.dst + (size_t)t * p.dst_stride;
  if (row == 0)
    for (int i = tid; i < JPEG_HEADER_BYTES; i += 256) f[i] = p.header.b[i];
  uint8_t* d = f + JPEG_HEADER_BYTES + s_sum[0][0] + 2ull * (unsigned long long)row;       // behind the RSTn of this row, if any
  if (row > 0 && tid == 0) { d[-2] = 0xFF; d[-1] = (uint8_t)(0xD0 + ((row - 1) & 7)); }
  const uint8_t* s = p.seg + ((size_t)t * p.rows + row) * p.slot;
  const int n = len[row];
  for (int i = tid; i < n; i += 256) d[i] = s[i];
  if (row == p.rows - 1 && tid == 0) { d[n] = 0xFF; d[n + 1] = 0xD9; }
}

}  // namespace rib
