// png.hip.h — lossless PNG of the folder driver's frames, encoded on the GPU (rib_png, include/rib.h).
//
// png.py (encode_host) states the file as an exact integer definition - one IDAT chunk per strip of 8 rows, a filter per row by
// the smallest sum of |int8|, runs at distance 1 as the only matches, the cheapest of K given Huffman tables per strip, an empty
// stored block between strips - and these kernels write the same bytes from uint8 HWC frames on the device.  Every rule below is
// png.py's; the host half (png_build_tables) restates canonical_codes, cl_symbols, cl_code_lengths and table_header line by line.
//
//   k_png_strips    grid (strips, T), 256 threads, n = rows * (1 + 3 W) bytes of dynamic LDS: a workgroup owns ONE strip.
//                     1. the five filters of every row are priced from the raw rows in global memory (the row above is the raw
//                        row, zero above row 0): five integer sums per thread, a wave reduction, an LDS add per wave;
//                     2. the chosen filter's bytes, behind the filter-type byte, go to LDS: the strip's n bytes, nothing else;
//                     3. a thread owns a contiguous piece of ceil(n / 256) bytes; a maximum scan of the pieces' last run start
//                        and a minimum scan of their first give every thread the start of the run that enters its piece and
//                        the end of the run that leaves it, so the tokens that START in a piece follow from arithmetic
//                        (png_walk) however long the run is;
//                     4. the walk once for the 286-bin histogram (integer LDS adds: order-independent) and the piece's Adler sums;
//                     5. the K tables priced (16 threads per table), the cheapest chosen, its codes copied to LDS;
//                     6. the walk again for the piece's bits, a scan of the 256 counts;
//                     7. the walk a third time, writing: a thread stores the dwords its bits cover completely straight into the
//                        strip's staging slot and ORs its share of a dword that holds a piece boundary into an LDS word owned by
//                        the first boundary inside that dword, which one thread stores afterwards - no global atomics, every
//                        byte stored once; thread 0 puts BFINAL and the header first, thread 255 end-of-block and the trailer;
//                     8. the chunk CRC: a thread per piece of the strip's bytes, each CRC shifted behind the bytes that follow
//                        it (multiplication by x^(8 n) mod P, zlib's crc32_combine) and XORed together; the Adler pair summed.
//                   The slot is png_slot_bytes(W) (the bound of png.max_bytes): never exceeded, and still checked on every store.
//   k_png_assemble  grid (strips, T), 256 threads: a workgroup sums the strip lengths of its frame in front of its own (and all of
//                   them: the file length), then copies its strip behind the prefix and the earlier chunks with its length, type
//                   and CRC; strip 0 also writes the prefix and lengths[t], the last strip combines the Adler pairs in closed form
//                   (A = 1 + sum (A_j - 1), B = sum B_j + (A_j - 1) * (bytes behind strip j), mod 65521) and writes the Adler
//                   chunk and IEND.  A frame that does not fit dst_stride writes nothing and gets length 0.
// No atomics on global memory, no floats, nothing depends on T or on the order in which workgroups run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace rib {

constexpr int PNG_STRIP_ROWS = 8;
constexpr int PNG_NSYM = 286;
constexpr int PNG_MAX_TABLES = 16;
constexpr int PNG_MAX_W = 4096;
constexpr int PNG_MAX_H = 65535;
constexpr int PNG_HEADER_BITS_BOUND = 2083;             // png.HEADER_BITS_BOUND: 17 + 19 * 3 + 287 * 7
constexpr int PNG_HDR_WORDS = (PNG_HEADER_BITS_BOUND + 31) / 32;
constexpr int PNG_PREFIX_BYTES = 47;                    // signature 8, IHDR 25, the zlib header's IDAT 14
constexpr uint32_t PNG_ADLER = 65521;
constexpr uint32_t PNG_CRC_POLY = 0xEDB88320u;

__host__ __device__ inline uint32_t png_crc_byte(uint32_t c, uint32_t byte) {      // one byte into the running (inverted) CRC
  c ^= byte;
#pragma unroll
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (PNG_CRC_POLY & (0u - (c & 1u)));
  return c;
}
__host__ __device__ inline uint32_t png_crc(const uint8_t* p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) c = png_crc_byte(c, p[i]);
  return c ^ 0xFFFFFFFFu;
}
// a(x) b(x) mod P in the reflected representation (bit 31 is x^0); zlib's multmodp with a fixed trip count
__device__ inline uint32_t png_multmodp(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = (b >> 1) ^ (PNG_CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}
// crc shifted behind `bytes` further bytes: crc32_combine(crc, 0, bytes) without the second operand
__device__ inline uint32_t png_crc_shift(uint32_t crc, uint32_t bytes) {
  uint32_t p = 1u << 31, sq = 1u << 23;                 // x^0; x^8
  for (; bytes; bytes >>= 1) {
    if (bytes & 1u) p = png_multmodp(sq, p);
    sq = png_multmodp(sq, sq);
  }
  return png_multmodp(p, crc);
}

inline size_t png_strip_data_bound(size_t n) { return (1 + (size_t)PNG_HEADER_BITS_BOUND + 9 * n + 9 + 10 + 7) / 8 + 4; }      // png.strip_bound - 12
inline size_t png_slot_bytes(int W) { return (png_strip_data_bound((size_t)PNG_STRIP_ROWS * (1 + 3 * (size_t)W)) + 15) / 16 * 16; }

// what the kernels read of K tables; built on the host (png_build_tables), one device copy per handle
struct PngDeviceTables {
  uint32_t code[PNG_MAX_TABLES][288];       // by symbol: bit-reversed code | length << 16
  uint32_t match[PNG_MAX_TABLES][260];      // by match length 3..258: length code, extra bits, the distance bit 0 | all their bits << 24
  uint32_t hdr[PNG_MAX_TABLES][PNG_HDR_WORDS];      // table_header, least significant bit first
  int32_t hdr_bits[PNG_MAX_TABLES];
  uint16_t lensym[260];                     // png.LEN_SYM
  int32_t K;
};

// ---- the host half: png.py's canonical_codes, cl_symbols, cl_code_lengths, table_header ----
namespace png_host {
constexpr int LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr int LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr int CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

inline uint32_t reverse_bits(uint32_t v, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1u); v >>= 1; }
  return r;
}

inline void canonical_codes(const int* len, int n, uint32_t* code) {      // RFC 1951 3.2.2
  int count[17] = {0}, next[17] = {0};
  for (int i = 0; i < n; ++i) if (len[i]) ++count[len[i]];
  int c = 0;
  for (int b = 1; b <= 15; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
  for (int i = 0; i < n; ++i) code[i] = len[i] ? (uint32_t)next[len[i]]++ : 0u;
}

struct ClSym { int sym, ebits, eval; };

inline std::vector<ClSym> cl_symbols(const int* len, int n) {
  std::vector<ClSym> out;
  for (int i = 0; i < n;) {
    const int v = len[i];
    int c = 1;
    while (i + c < n && len[i + c] == v) ++c;
    i += c;
    if (v == 0) {
      while (c >= 11) { const int r = c < 138 ? c : 138; out.push_back({18, 7, r - 11}); c -= r; }
      while (c >= 3) { const int r = c < 10 ? c : 10; out.push_back({17, 3, r - 3}); c -= r; }
    } else {
      out.push_back({v, 0, 0});
      --c;
      while (c >= 3) { const int r = c < 6 ? c : 6; out.push_back({16, 2, r - 3}); c -= r; }
    }
    for (; c > 0; --c) out.push_back({v, 0, 0});
  }
  return out;
}

struct ClSearch {
  static constexpr int LIMIT = 7;
  static constexpr long long INF = 1ll << 60;
  int u = 0;
  long long f[19];
  long long memo_cost[LIMIT + 1][20][40];
  int memo_n[LIMIT + 1][20][40];
  long long sum(int a, int b) const { long long s = 0; for (int i = a; i < b; ++i) s += f[i]; return s; }
  long long best(int level, int i, int avail, int* leaves) {
    const int rem = u - i;
    if (avail > rem || rem > (avail << (LIMIT - level))) { *leaves = 0; return INF; }
    if (level == LIMIT) { *leaves = rem; return (long long)level * sum(i, u); }
    if (memo_n[level][i][avail] < 0) {
      long long rc = INF;
      int rn = 0;
      const int top = avail < rem ? avail : rem;
      for (int n = 0; n <= top; ++n) {
        if (n == rem && n != avail) continue;
        int dummy;
        long long c = n < rem ? best(level + 1, i + n, 2 * (avail - n), &dummy) : 0;
        if (c >= INF) continue;
        c += (long long)level * sum(i, i + n);
        if (c < rc) { rc = c; rn = n; }
      }
      memo_cost[level][i][avail] = rc;
      memo_n[level][i][avail] = rn;
    }
    *leaves = memo_n[level][i][avail];
    return memo_cost[level][i][avail];
  }
};

inline void cl_code_lengths(const int* freq, int* lengths) {
  int used[19], u = 0;
  for (int s = 0; s < 19; ++s) if (freq[s]) used[u++] = s;
  for (int a = 1; a < u; ++a)                              // by (-freq, symbol): a stable insertion sort by falling frequency
    for (int b = a; b > 0 && freq[used[b]] > freq[used[b - 1]]; --b) { const int x = used[b]; used[b] = used[b - 1]; used[b - 1] = x; }
  ClSearch* S = new ClSearch;
  S->u = u;
  for (int i = 0; i < u; ++i) S->f[i] = freq[used[i]];
  for (auto& a : S->memo_n) for (auto& b : a) for (int& c : b) c = -1;
  for (int s = 0; s < 19; ++s) lengths[s] = 0;
  int level = 1, i = 0, avail = 2;
  while (i < u) {
    int n;
    (void)S->best(level, i, avail, &n);
    for (int k = i; k < i + n; ++k) lengths[used[k]] = level;
    i += n; avail = 2 * (avail - n); ++level;
  }
  delete S;
}

// table_header as bits in stream order
inline std::vector<uint8_t> table_header(const uint8_t* lengths) {
  int len[PNG_NSYM + 1];
  for (int i = 0; i < PNG_NSYM; ++i) len[i] = lengths[i];
  len[PNG_NSYM] = 1;
  const std::vector<ClSym> syms = cl_symbols(len, PNG_NSYM + 1);
  int freq[19] = {0}, cl[19];
  for (const ClSym& s : syms) ++freq[s.sym];
  cl_code_lengths(freq, cl);
  uint32_t codes[19];
  canonical_codes(cl, 19, codes);
  int hclen = 4;
  for (int i = 0; i < 19; ++i) if (cl[CL_ORDER[i]]) hclen = i + 1 > hclen ? i + 1 : hclen;
  std::vector<uint8_t> bits;
  auto put = [&](uint32_t v, int n) { for (int b = 0; b < n; ++b) bits.push_back((uint8_t)((v >> b) & 1u)); };
  put(2, 2); put(29, 5); put(0, 5); put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) put((uint32_t)cl[CL_ORDER[i]], 3);
  for (const ClSym& s : syms) {
    put(reverse_bits(codes[s.sym], cl[s.sym]), cl[s.sym]);
    if (s.ebits) put((uint32_t)s.eval, s.ebits);
  }
  return bits;
}
}  // namespace png_host

// png.check_tables, then everything the kernels read; false with a text when the tables are refused
inline bool png_build_tables(const uint8_t* lengths, int K, PngDeviceTables* t, std::string* err) {
  using namespace png_host;
  if (K < 1 || K > PNG_MAX_TABLES) { *err = "K must lie in 1..16"; return false; }
  memset(t, 0, sizeof *t);
  t->K = K;
  for (int L = 3; L <= 258; ++L) {
    int s = 28;
    if (L < 258) { s = 0; while (s + 1 < 28 && LEN_BASE[s + 1] <= L) ++s; }
    t->lensym[L] = (uint16_t)(257 + s);
  }
  for (int k = 0; k < K; ++k) {
    const uint8_t* l = lengths + (size_t)k * PNG_NSYM;
    long long kraft = 0;
    int len[PNG_NSYM];
    for (int s = 0; s < PNG_NSYM; ++s) {
      if (l[s] < 1 || l[s] > 15) { *err = "table " + std::to_string(k) + ": every code length must lie in 1..15"; return false; }
      if (k == 0 && l[s] > 9) { *err = "table 0 must be flat: every length at most 9"; return false; }
      kraft += 1ll << (15 - l[s]);
      len[s] = l[s];
    }
    if (kraft != 1ll << 15) { *err = "table " + std::to_string(k) + " is not a complete prefix code"; return false; }
    uint32_t codes[PNG_NSYM];
    canonical_codes(len, PNG_NSYM, codes);
    for (int s = 0; s < PNG_NSYM; ++s) t->code[k][s] = reverse_bits(codes[s], len[s]) | ((uint32_t)len[s] << 16);
    for (int L = 3; L <= 258; ++L) {
      const int sym = t->lensym[L], si = sym - 257;
      const uint32_t c = t->code[k][sym] & 0xFFFFu;
      const int cl = len[sym], eb = LEN_EXTRA[si];
      t->match[k][L] = (c | ((uint32_t)(L - LEN_BASE[si]) << cl)) | ((uint32_t)(cl + eb + 1) << 24);
    }
    const std::vector<uint8_t> bits = table_header(l);
    if ((int)bits.size() > PNG_HEADER_BITS_BOUND) { *err = "table header longer than its bound"; return false; }
    t->hdr_bits[k] = (int32_t)bits.size();
    for (size_t b = 0; b < bits.size(); ++b) t->hdr[k][b >> 5] |= (uint32_t)bits[b] << (b & 31);
  }
  return true;
}

// png.prefix: signature, IHDR, the IDAT chunk of the zlib header
inline void png_make_prefix(uint8_t* p, int H, int W) {
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  memcpy(p, sig, 8);
  const uint8_t ihdr[21] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', (uint8_t)(W >> 24), (uint8_t)(W >> 16), (uint8_t)(W >> 8), (uint8_t)W,
                            (uint8_t)(H >> 24), (uint8_t)(H >> 16), (uint8_t)(H >> 8), (uint8_t)H, 8, 2, 0, 0, 0};
  memcpy(p + 8, ihdr, 21);
  uint32_t c = png_crc(p + 12, 17);
  p[29] = (uint8_t)(c >> 24); p[30] = (uint8_t)(c >> 16); p[31] = (uint8_t)(c >> 8); p[32] = (uint8_t)c;
  const uint8_t z[10] = {0, 0, 0, 2, 'I', 'D', 'A', 'T', 0x78, 0x01};
  memcpy(p + 33, z, 10);
  c = png_crc(p + 37, 6);
  p[43] = (uint8_t)(c >> 24); p[44] = (uint8_t)(c >> 16); p[45] = (uint8_t)(c >> 8); p[46] = (uint8_t)c;
}

struct PngParams {
  const uint8_t* src;            // [T, H, W, 3]
  const PngDeviceTables* tab;
  uint8_t* slots;                // [T, strips] slots of `slot` bytes: a strip's deflate bytes
  int32_t* meta;                 // [T, strips, 4]: bytes (-1: the slot would have been exceeded), chunk CRC, Adler A, Adler B
  int H, W, strips;
  uint32_t slot;                 // a multiple of 16
};

__device__ inline int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ inline int png_abs8(int v) { v &= 255; return v >= 128 ? 256 - v : v; }
__device__ inline int png_filter(int ft, int x, int a, int b, int c) {
  switch (ft) {
    case 0: return x;
    case 1: return (x - a) & 255;
    case 2: return (x - b) & 255;
    case 3: return (x - ((a + b) >> 1)) & 255;
    default: return (x - png_paeth(a, b, c)) & 255;
  }
}

// The tokens that START at positions c0 <= p < c1 of the strip's bytes d[0..n), in order.  run_in: the start of the run that holds
// c0 when d[c0] continues d[c0 - 1]; run_out: the end of the run that holds c1 - 1 when d[c1] continues it.  A run [s, e) of R
// bytes codes a literal at s, matches of 258 at s + 1 + 258 i while at least 4 bytes remain behind them... exactly: with m = R - 1,
// full = m / 258 matches of 258, then r = m - 258 full: one match of r at tb = s + 1 + 258 full if r >= 4, else r literals from tb.
template <typename F>
__device__ inline void png_walk(const uint8_t* d, int n, int c0, int c1, int run_in, int run_out, F& f) {
  int p = c0;
  while (p < c1) {
    const int v = d[p];
    int s = p;
    if (p == c0 && p > 0 && d[p - 1] == v) s = run_in;
    int e = p + 1;
    while (e < c1 && d[e] == v) ++e;
    if (e == c1 && c1 < n && d[c1] == v) e = run_out;
    const int hi = e < c1 ? e : c1;
    if (s == p) f.lit(v, 1);
    const int m = e - s - 1, full = m / 258, r = m - full * 258;
    int i = p > s + 1 ? (p - s - 1 + 257) / 258 : 0;
    for (; i < full && s + 1 + 258 * i < hi; ++i) f.match(258);
    const int tb = s + 1 + 258 * full;
    if (r >= 4) {
      if (tb >= p && tb < hi) f.match(r);
    } else {
      const int lo = tb > p ? tb : p;
      const int cnt = (tb + r < hi ? tb + r : hi) - lo;
      if (cnt > 0) f.lit(v, cnt);
    }
    p = hi;
  }
}

struct PngHistWalk {
  uint32_t* hist;
  const uint16_t* lensym;
  __device__ void lit(int v, int cnt) { atomicAdd(&hist[v], (uint32_t)cnt); }
  __device__ void match(int L) { atomicAdd(&hist[lensym[L]], 1u); }
};
struct PngCountWalk {
  const uint32_t* code;
  const uint32_t* mt;
  uint32_t bits;
  __device__ void lit(int v, int cnt) { bits += (uint32_t)cnt * (code[v] >> 16); }
  __device__ void match(int L) { bits += mt[L] >> 24; }
};
// a thread's bits [b0, b1) of the strip, least significant bit first: dwords it covers completely go straight to the slot, its
// share of a dword with a piece boundary inside is ORed into the LDS word of the FIRST boundary inside that dword
struct PngEmitWalk {
  const uint32_t* code;
  const uint32_t* mt;
  uint32_t* out;
  uint32_t* part;
  const uint32_t* b;
  uint32_t slotw, b0, b1, wi;
  int t, n;
  uint64_t acc;
  __device__ void start() { wi = b0 >> 5; n = (int)(b0 & 31u); acc = 0; }
  __device__ void flush(uint32_t w) {
    const uint32_t lo = wi * 32u;
    if (lo >= b0 && lo + 32u <= b1) {
      if (wi < slotw) out[wi] = w;
    } else {
      int i = t + 1;
      if (b0 > lo) { i = t; while (i > 1 && b[i - 1] > lo) --i; }
      atomicOr(&part[i], w);
    }
  }
  __device__ void put(uint32_t v, int len) {             // len <= 24, n < 32
    acc |= (uint64_t)v << n;
    n += len;
    if (n >= 32) { flush((uint32_t)acc); acc >>= 32; n -= 32; ++wi; }
  }
  __device__ void finish() { if (n > 0) flush((uint32_t)acc); }
  __device__ void lit(int v, int cnt) { const uint32_t e = code[v]; for (; cnt > 0; --cnt) put(e & 0xFFFFu, (int)(e >> 16)); }
  __device__ void match(int L) { const uint32_t e = mt[L]; put(e & 0xFFFFFFu, (int)(e >> 24)); }
};

__global__ __launch_bounds__(256) void k_png_strips(PngParams p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_d[];      // the strip's filtered bytes
  __shared__ uint32_t s_hist[288];
  __shared__ uint32_t s_code[288];
  __shared__ uint32_t s_match[260];
  __shared__ uint32_t s_b[257];            // bit offsets of the pieces; s_b[256]: the strip's bits, trailer included
  __shared__ uint32_t s_part[257];
  __shared__ int s_run[2][256];
  __shared__ int s_cost[PNG_STRIP_ROWS][5];
  __shared__ int s_ft[PNG_STRIP_ROWS];
  __shared__ uint32_t s_costk[PNG_MAX_TABLES];
  __shared__ uint32_t s_sum[3];            // Adler sums, CRC
  __shared__ int s_k;
  uint16_t* const s_lensym = reinterpret_cast<uint16_t*>(s_match);       // png.LEN_SYM, until the chosen table's matches take its place (step 5)
  uint32_t* const s_scan = reinterpret_cast<uint32_t*>(s_run[0]);        // the pieces' bit counts, once the run scans have been read (step 6)
  const int tid = threadIdx.x, strip = blockIdx.x, t = blockIdx.y;
  const int lane = tid & 63;
  const int H = p.H, rowB = 3 * p.W;
  const int y0 = strip * PNG_STRIP_ROWS;
  const int rows = min(PNG_STRIP_ROWS, H - y0);
  const int n = rows * (1 + rowB);
  const int K = p.tab->K;
  const bool last = strip == p.strips - 1;
  const uint8_t* img = p.src + (size_t)t * H * rowB;

  for (int i = tid; i < 288; i += 256) s_hist[i] = 0;
  for (int i = tid; i < 257; i += 256) s_part[i] = 0;
  for (int i = tid; i < 260; i += 256) s_lensym[i] = p.tab->lensym[i];
  if (tid < PNG_STRIP_ROWS * 5) (&s_cost[0][0])[tid] = 0;
  if (tid < PNG_MAX_TABLES) s_costk[tid] = tid < K ? (uint32_t)p.tab->hdr_bits[tid] : 0xFFFFFFFFu;
  if (tid < 3) s_sum[tid] = 0;
  __syncthreads();

  // ---- 1. the five filters of every row, priced ----
  for (int r = 0; r < rows; ++r) {
    const uint8_t* cur = img + (size_t)(y0 + r) * rowB;
    const bool has_up = y0 + r > 0;
    const uint8_t* up = cur - (has_up ? rowB : 0);
    int c[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < rowB; i += 256) {
      const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, cc = (has_up && i >= 3) ? up[i - 3] : 0;
      c[0] += png_abs8(x);
      c[1] += png_abs8(x - a);
      c[2] += png_abs8(x - b);
      c[3] += png_abs8(x - ((a + b) >> 1));
      c[4] += png_abs8(x - png_paeth(a, b, cc));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      int v = c[f];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
      if (lane == 0) atomicAdd(&s_cost[r][f], v);
    }
  }
  __syncthreads();
  if (tid < rows) {
    int ft = 0;
    for (int f = 1; f < 5; ++f)
      if (s_cost[tid][f] < s_cost[tid][ft]) ft = f;      // a tie: the lower type
    s_ft[tid] = ft;
  }
  __syncthreads();
  // ---- 2. the chosen filter's bytes -> LDS ----
  for (int r = 0; r < rows; ++r) {
    const uint8_t* cur = img + (size_t)(y0 + r) * rowB;
    const bool has_up = y0 + r > 0;
    const uint8_t* up = cur - (has_up ? rowB : 0);
    const int ft = s_ft[r];
    uint8_t* o = s_d + r * (1 + rowB);
    if (tid == 0) o[0] = (uint8_t)ft;
    for (int i = tid; i < rowB; i += 256) {
      const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, cc = (has_up && i >= 3) ? up[i - 3] : 0;
      o[1 + i] = (uint8_t)png_filter(ft, x, a, b, cc);
    }
  }
  __syncthreads();

  // ---- 3. pieces and the runs that cross them ----
  const int C = (n + 255) / 256;
  const int c0 = min(tid * C, n), c1 = min(c0 + C, n);
  {
    int run_last = -1, run_first = n;
    for (int q = c0; q < c1; ++q)
      if (q == 0 || s_d[q] != s_d[q - 1]) {
        if (run_first == n) run_first = q;
        run_last = q;
      }
    s_run[0][tid] = run_last;
    s_run[1][tid] = run_first;
  }
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int a = tid >= off ? s_run[0][tid - off] : -1;
    const int b = tid + off < 256 ? s_run[1][tid + off] : n;
    __syncthreads();
    s_run[0][tid] = max(s_run[0][tid], a);
    s_run[1][tid] = min(s_run[1][tid], b);
    __syncthreads();
  }
  const int run_in = tid > 0 ? s_run[0][tid - 1] : 0;
  const int run_out = tid < 255 ? s_run[1][tid + 1] : n;

  // ---- 4. histogram, Adler sums ----
  {
    PngHistWalk hw{s_hist, s_lensym};
    png_walk(s_d, n, c0, c1, run_in, run_out, hw);
    if (tid == 0) atomicAdd(&s_hist[256], 1u);
    unsigned long long sa = 0, sb = 0;
    for (int q = c0; q < c1; ++q) {
      const unsigned long long v = s_d[q];
      sa += v;
      sb += v * (unsigned long long)(n - q);
    }
    if (c1 > c0) {
      atomicAdd(&s_sum[0], (uint32_t)(sa % PNG_ADLER));
      atomicAdd(&s_sum[1], (uint32_t)(sb % PNG_ADLER));
    }
  }
  __syncthreads();
  // ---- 5. the cheapest table ----
  {
    const int k = tid >> 4, sub = tid & 15;
    if (k < K) {
      uint32_t sum = 0;
      for (int s = sub; s < PNG_NSYM; s += 16) sum += s_hist[s] * (p.tab->code[k][s] >> 16);
      atomicAdd(&s_costk[k], sum);
    }
  }
  __syncthreads();
  if (tid == 0) {
    int k = 0;
    for (int j = 1; j < K; ++j)
      if (s_costk[j] < s_costk[k]) k = j;                 // a tie: the lower k
    s_k = k;
  }
  __syncthreads();
  const int k = s_k;
  for (int i = tid; i < PNG_NSYM; i += 256) s_code[i] = p.tab->code[k][i];
  for (int i = tid; i < 260; i += 256) s_match[i] = p.tab->match[k][i];
  __syncthreads();
  // ---- 6. bits per piece, their offsets ----
  const int hdr_bits = p.tab->hdr_bits[k];
  {
    PngCountWalk cw{s_code, s_match, 0u};
    png_walk(s_d, n, c0, c1, run_in, run_out, cw);
    if (tid == 0) cw.bits += 1u + (uint32_t)hdr_bits;
    if (tid == 255) cw.bits += s_code[256] >> 16;
    s_scan[tid] = cw.bits;
  }
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const uint32_t a = tid >= off ? s_scan[tid - off] : 0u;
    __syncthreads();
    s_scan[tid] += a;
    __syncthreads();
  }
  const uint32_t body = s_scan[255];                     // BFINAL .. end-of-block
  const uint32_t end = last ? (body + 7u) & ~7u : ((body + 3u + 7u) & ~7u) + 32u;
  s_b[tid + 1] = tid == 255 ? end : s_scan[tid];
  if (tid == 0) s_b[0] = 0;
  __syncthreads();
  // ---- 7. the bits ----
  uint32_t* const out = reinterpret_cast<uint32_t*>(p.slots + ((size_t)t * p.strips + strip) * p.slot);
  const uint32_t slotw = p.slot >> 2;
  {
    PngEmitWalk ew;
    ew.code = s_code; ew.mt = s_match; ew.out = out; ew.part = s_part; ew.b = s_b; ew.slotw = slotw;
    ew.b0 = s_b[tid]; ew.b1 = s_b[tid + 1]; ew.t = tid;
    if (ew.b1 > ew.b0) {
      ew.start();
      if (tid == 0) {
        ew.put(last ? 1u : 0u, 1);
        const uint32_t* hw = p.tab->hdr[k];
        for (int q = 0; q < hdr_bits; q += 16) {
          const int len = min(16, hdr_bits - q);
          ew.put((hw[q >> 5] >> (q & 31)) & ((1u << len) - 1u), len);
        }
      }
      png_walk(s_d, n, c0, c1, run_in, run_out, ew);
      if (tid == 255) {
        ew.put(s_code[256] & 0xFFFFu, (int)(s_code[256] >> 16));
        if (last) {
          ew.put(0u, (int)(end - body));
        } else {
          ew.put(0u, (int)(end - 32u - body));           // the stored block's 000 and the padding: 3..10 zero bits
          ew.put(0u, 16);
          ew.put(0xFFFFu, 16);
        }
      }
      ew.finish();
    }
  }
  __syncthreads();
  for (int i = tid + 1; i <= 256; i += 256) {
    const uint32_t bi = s_b[i];
    if (bi & 31u) {
      const uint32_t w = bi >> 5;
      if ((i == 1 || s_b[i - 1] <= w * 32u) && w < slotw) out[w] = s_part[i];
    }
  }
  __syncthreads();
  // ---- 8. the chunk CRC over "IDAT" and the strip's bytes ----
  const uint32_t nbytes = end >> 3;
  const bool fits = nbytes <= p.slot;
  if (fits) {
    const uint32_t P = ((nbytes + 255u) / 256u + 3u) & ~3u;
    const uint32_t q0 = min((uint32_t)tid * P, nbytes), q1 = min(q0 + P, nbytes);
    if (q1 > q0) {
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t q = q0; q < q1; q += 4) {
        const uint32_t w = out[q >> 2];
        const uint32_t m = min(4u, q1 - q);
        for (uint32_t j = 0; j < m; ++j) c = png_crc_byte(c, (w >> (8 * j)) & 255u);
      }
      atomicXor(&s_sum[2], png_crc_shift(c ^ 0xFFFFFFFFu, nbytes - q1));
    }
    if (tid == 255) {
      const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
      atomicXor(&s_sum[2], png_crc_shift(png_crc(idat, 4), nbytes));
    }
  }
  __syncthreads();
  if (tid == 0) {
    int32_t* m = p.meta + ((size_t)t * p.strips + strip) * 4;
    m[0] = fits ? (int32_t)nbytes : -1;
    m[1] = (int32_t)s_sum[2];
    m[2] = (int32_t)((1u + s_sum[0]) % PNG_ADLER);
    m[3] = (int32_t)(((uint32_t)(n % (int)PNG_ADLER) + s_sum[1]) % PNG_ADLER);
  }
}

struct PngAssembleParams {
  const uint8_t* slots;
  const int32_t* meta;
  uint8_t* dst;
  int32_t* lengths;
  size_t dst_stride;
  int H, W, strips;
  uint32_t slot;
  uint8_t prefix[PNG_PREFIX_BYTES + 1];
};

__device__ inline void png_put_be32(uint8_t* d, uint32_t v) {
  d[0] = (uint8_t)(v >> 24); d[1] = (uint8_t)(v >> 16); d[2] = (uint8_t)(v >> 8); d[3] = (uint8_t)v;
}

__global__ __launch_bounds__(256) void k_png_assemble(PngAssembleParams p) {
  __shared__ unsigned long long s_sum[4][256];
  __shared__ int s_bad[256];
  const int tid = threadIdx.x, row = blockIdx.x, t = blockIdx.y;
  const int32_t* meta = p.meta + (size_t)t * p.strips * 4;
  const unsigned long long rowN = 1ull + 3ull * (unsigned long long)p.W, N = rowN * (unsigned long long)p.H;
  unsigned long long before = 0, all = 0, sa = 0, sb = 0;
  int bad = 0;
  for (int r = tid; r < p.strips; r += 256) {
    const int32_t l = meta[4 * r];
    if (l < 0) { bad = 1; continue; }
    all += (unsigned long long)l;
    if (r < row) before += (unsigned long long)l;
    const unsigned long long a1 = ((unsigned long long)meta[4 * r + 2] + PNG_ADLER - 1ull) % PNG_ADLER;       // A_r - 1
    const unsigned long long endr = (unsigned long long)min((r + 1) * PNG_STRIP_ROWS, p.H) * rowN;
    sa = (sa + a1) % PNG_ADLER;
    sb = (sb + (unsigned long long)meta[4 * r + 3] + a1 * ((N - endr) % PNG_ADLER)) % PNG_ADLER;
  }
  s_sum[0][tid] = before; s_sum[1][tid] = all; s_sum[2][tid] = sa; s_sum[3][tid] = sb; s_bad[tid] = bad;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {                    // integer sums: the order does not matter
    if (tid < s) {
      s_sum[0][tid] += s_sum[0][tid + s]; s_sum[1][tid] += s_sum[1][tid + s];
      s_sum[2][tid] += s_sum[2][tid + s]; s_sum[3][tid] += s_sum[3][tid + s];
      s_bad[tid] |= s_bad[tid + s];
    }
    __syncthreads();
  }
  const unsigned long long total = (unsigned long long)PNG_PREFIX_BYTES + s_sum[1][0] + 12ull * (unsigned long long)p.strips + 16ull + 12ull;
  const bool refused = s_bad[0] || total > (unsigned long long)p.dst_stride;
  if (row == 0 && tid == 0) p.lengths[t] = refused ? 0 : (int32_t)total;
  if (refused) return;
  uint8_t* f = p.dst + (size_t)t * p.dst_stride;
  if (row == 0)
    for (int i = tid; i < PNG_PREFIX_BYTES; i += 256) f[i] = p.prefix[i];
  uint8_t* d = f + PNG_PREFIX_BYTES + s_sum[0][0] + 12ull * (unsigned long long)row;
  const uint8_t* s = p.slots + ((size_t)t * p.strips + row) * p.slot;
  const int n = meta[4 * row];
  if (tid == 0) {
    png_put_be32(d, (uint32_t)n);
    d[4] = 'I'; d[5] = 'D'; d[6] = 'A'; d[7] = 'T';
    png_put_be32(d + 8 + n, (uint32_t)meta[4 * row + 1]);
  }
  for (int i = tid; i < n; i += 256) d[8 + i] = s[i];
  if (row == p.strips - 1 && tid == 0) {
    uint8_t* e = d + 12 + n;
    const uint32_t A = (uint32_t)((1ull + s_sum[2][0]) % PNG_ADLER), B = (uint32_t)(s_sum[3][0] % PNG_ADLER);
    png_put_be32(e, 4u);
    e[4] = 'I'; e[5] = 'D'; e[6] = 'A'; e[7] = 'T';
    png_put_be32(e + 8, (B << 16) | A);
    png_put_be32(e + 12, png_crc(e + 4, 8));
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    for (int i = 0; i < 12; ++i) e[16 + i] = iend[i];
  }
}

}  // namespace rib
