// frame_kernels.hip -- frame I/O: the kernels that move pixels between the caller's frames and the tiles a plan works on (gfx950, wave64).
// None of them is an op of a plan; film_engine.cpp and film_stream.cpp call the four launchers at the end of this file and film_launch_frame_histogram / film_launch_frame_diff / film_launch_segment_copy, which stand beside their kernels.
//
//   frame_to_tiles<OVERLAP>             _pad_to_align + image_to_patches, float32 frames    eval/interpolator.py:30-63, :66-104
//   frame_u8_to_tiles<OVERLAP>          the same on 8-bit RGB frames: float32(byte) / 255   eval/util.py read_image
//   frame_yuv_to_tiles<OVERLAP,LAYOUT>  the same on Y'CbCr frames (4:2:0, 4:2:2, 4:4:4; 8 / 10 bit)  include/film_hip.h, "The 4:2:0 arithmetic", "The 10-bit ...", "The 4:2:2 and 4:4:4 ..."
//   tiles_to_frame                    crop + patches_to_image                             eval/interpolator.py:107-126, :192-206
//   blend_tiles                         crop + cross-fade of overlapped tiles               include/film_hip.h, "block_overlap_h"
//   to_uint8                            clip(x * 255, 0, 255) + 0.5, truncated              eval/util.py:51-52 (write_image)
//   rgb_to_yuv<LAYOUT>                  float32 RGB -> the planes of one Y'CbCr frame       the same three sections
//   frame_histogram<LAYOUT>            3 x 256 counters of a frame's 8-bit sample codes    include/film_hip.h, "Scene cuts"
//   frame_diff<LAYOUT>                 the 8 x 8 block SADs of two frames, per plane       include/film_hip.h, "Duplicate frames"
//   segment_copy                       a table of float segments, device to device         film_kernels.h, SegmentTable
//
// OVERLAP: the tile's content is the patch grown by the overlap, from film_tile_origin (options "block_overlap_h" / "block_overlap_w").
// LAYOUT: a FILM_PIX_* value.  The Y'CbCr cut and quantiser are written once over YuvLayout<LAYOUT>, which states what a layout decides: the sample
// type and how many fit a 32-bit word, the chroma shifts (SX, SY) = (1, 1) for 4:2:0, (1, 0) for 4:2:2, (0, 0) for 4:4:4, planar or semi-planar
// chroma, where the code sits in a sample, the largest code and the chroma midpoint, the constants the kernels take and the aligned multi-sample
// load.  What only one depth or one subsampling does stands behind `if constexpr`: the 8-bit LDS tables against the 10-bit division, P010's
// direct reads of its CbCr pair words, the four chroma samples per group of 4:4:4, the chroma means of the quantiser.
//
// This file is compiled with -ffp-contract=off, like misc_kernels.hip: the cross-fade, the colour matrices and the quantisers are specified
// as separate multiply / add operations (one rounding each), so a*b+c must not become an fma here.
#include <type_traits>

#include "film_kernels.h"

namespace {

// how every kernel of this file is launched ("host", below)
template <class... P, class... A>
hipError_t launch_units(void (*kernel)(P...), int64_t units, hipStream_t s, const A&... args);

// ---- what the cuts share -------------------------------------------------------------------------------------------------------
// Row r of the tile buffer: its row y inside the padded tile, and the tile's frame b and block (ty, tx) of that frame.
__device__ __forceinline__ void tile_row(const TileMapParams& p, int64_t r, int& y, int& b, int& ty, int& tx) {
  y = (int)(r % p.TH);
  const int n = (int)(r / p.TH) + p.tile0;
  b = n / (p.bh * p.bw);
  const int t = n % (p.bh * p.bw);
  ty = t / p.bw; tx = t % p.bw;
}

// The content of tile (ty, tx): rows x cols pixels of the frame from (row0, col0), which lie at (oy, ox) of the padded tile.  Without overlap
// these are the patches of the reference (tf.image.pad_to_bounding_box pads them with zeros).
// (Four accessors, not one function: each value is formed where the kernel uses it, which keeps the kernels' instruction streams as they were.)
template <bool OVERLAP> struct TileContent {
  static __device__ __forceinline__ int rows(const TileMapParams& p) { return OVERLAP ? p.eh : p.ph; }
  static __device__ __forceinline__ int cols(const TileMapParams& p) { return OVERLAP ? p.ew : p.pw; }
  static __device__ __forceinline__ int row0(const TileMapParams& p, int ty) { return OVERLAP ? film_tile_origin(ty, p.ph, p.ovy, p.H, p.eh) : ty * p.ph; }
  static __device__ __forceinline__ int col0(const TileMapParams& p, int tx) { return OVERLAP ? film_tile_origin(tx, p.pw, p.ovx, p.W, p.ew) : tx * p.pw; }
};

// n <= 7 bytes from p as the low bytes of a 64-bit value, read as the one or two ALIGNED 32-bit words that hold them: every word read
// holds at least one of the bytes asked for
__device__ __forceinline__ uint64_t load_bytes_aligned(const uint8_t* p, int n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const unsigned off = (unsigned)(a & 3);
  uint64_t v = wp[0];
  if (off + (unsigned)n > 4) v |= (uint64_t)wp[1] << 32;
  return v >> (off * 8);
}
__device__ __forceinline__ float clip01(float v) {
  v = v < 0.f ? 0.f : v;      // max(v, 0) then min(v, 1)
  return v > 1.f ? 1.f : v;
}
// the quantiser of every way out: clip(v, 0, MAX) + 0.5, truncated (np.clip = minimum(maximum(x, 0), MAX)); MAX = 255, or 1023 for 10-bit codes
template <int MAX> __device__ __forceinline__ uint32_t quantise(float v) {
  v = v < 0.f ? 0.f : v;
  v = v > (float)MAX ? (float)MAX : v;
  return (uint32_t)(v + 0.5f);
}

// ---- Interpolator.__call__ data movement ----------------------------------------------------------------
// thread = one float of the tile buffer (frame_to_tiles) / of the frame (tiles_to_frame); both sides are
// contiguous in x*3+c, so consecutive threads read and write consecutive floats of a row.
template <bool OVERLAP>
__global__ __launch_bounds__(256) void frame_to_tiles_kernel(TileMapParams p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int row = p.TW * 3;
  const int64_t total = (int64_t)p.ntiles * p.TH * row;
  if (i >= total) return;
  const int xc = (int)(i % row);
  using C = TileContent<OVERLAP>;
  int y, b, ty, tx;
  tile_row(p, i / row, y, b, ty, tx);
  const int sy = y - p.oy, sxc = xc - p.ox * 3;
  float v = 0.f;  // tf.image.pad_to_bounding_box pads with zeros
  if (sy >= 0 && sy < C::rows(p) && sxc >= 0 && sxc < C::cols(p) * 3)
    v = p.src[(((int64_t)b * p.H + C::row0(p, ty) + sy) * p.W + C::col0(p, tx)) * 3 + sxc];
  p.dst[i] = v;
}

__global__ __launch_bounds__(256) void tiles_to_frame_kernel(TileMapParams p) {
  // thread = one float of the patches [tile0, tile0 + ntiles) as they lie in the frame
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int row = p.pw * 3;
  const int64_t total = (int64_t)p.ntiles * p.ph * row;
  if (i >= total) return;
  const int xc = (int)(i % row);
  const int64_t r = i / row;
  const int y = (int)(r % p.ph);
  const int ln = (int)(r / p.ph);
  const int n = ln + p.tile0;
  const int b = n / (p.bh * p.bw), t = n % (p.bh * p.bw);
  const int ty = t / p.bw, tx = t % p.bw;
  const float v = p.src[(((int64_t)ln * p.TH + p.oy + y) * p.TW + p.ox) * 3 + xc];
  p.dst[(((int64_t)b * p.H + ty * p.ph + y) * p.W + tx * p.pw) * 3 + xc] = v;
}

// ---- the cut on an 8-bit frame (film_stream_push, FILM_PIX_U8) ------------------------------------------------------------
// float32(byte) / 255.0f for every byte value, divided on the HOST (IEEE, = numpy's astype(float32) / 255 and eval/util.py read_image): the
// kernel looks the quotient up, so no device division and no reciprocal decides a bit.  Passed by value (1 KB of kernel arguments).
struct U8Table { float v[256]; };

// frame_to_tiles_kernel on a frame of bytes: p.src points at uint8 [B][H][W][3].  thread = twelve consecutive values (four pixels) of one
// row of the tile buffer, the same tile-row-major order as the float kernel.  A group that lies
// wholly inside the tile's content is read as the three or four ALIGNED 32-bit words that hold its twelve bytes (a row of W * 3 bytes
// starts at any byte offset; every word read holds at least one byte of the group, so none lies outside the frame's pages) and shifted
// into place; a group that touches the padding or the end of the row goes byte by byte.  Padding is written as zeros; the twelve floats
// leave as three 16-byte stores where the row pitch allows.
template <bool OVERLAP>
__global__ __launch_bounds__(256) void frame_u8_to_tiles_kernel(TileMapParams p, U8Table tab) {
  __shared__ float lut[256];
  lut[threadIdx.x] = tab.v[threadIdx.x];
  __syncthreads();
  const int row = p.TW * 3;
  const int groups = (row + 11) / 12;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)p.ntiles * p.TH * groups) return;
  const int xc0 = (int)(g % groups) * 12;
  const int64_t r = g / groups;               // row of the tile buffer
  using C = TileContent<OVERLAP>;
  int y, b, ty, tx;
  tile_row(p, r, y, b, ty, tx);
  const int ch = C::rows(p), cw3 = C::cols(p) * 3;                           // the tile's content: rows, values per row
  const int sy = y - p.oy, s0 = xc0 - p.ox * 3;                              // content row, content value of the group's first value
  float v[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) v[j] = 0.f;   // tf.image.pad_to_bounding_box pads with zeros
  if (sy >= 0 && sy < ch && s0 + 12 > 0 && s0 < cw3) {
    const int fy = C::row0(p, ty) + sy, fx = C::col0(p, tx);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(p.src) + (((int64_t)b * p.H + fy) * p.W + fx) * 3;   // content value 0 of this row
    if (s0 >= 0 && s0 + 12 <= cw3) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(src + s0);
      const uint32_t* wp = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
      const unsigned sh = (unsigned)(a & 3) * 8;
      uint32_t w[3] = {wp[0], wp[1], wp[2]};
      if (sh) {
        const uint32_t w3 = wp[3];
        w[0] = (w[0] >> sh) | (w[1] << (32 - sh));
        w[1] = (w[1] >> sh) | (w[2] << (32 - sh));
        w[2] = (w[2] >> sh) | (w3 << (32 - sh));
      }
#pragma unroll
      for (int j = 0; j < 12; ++j) v[j] = lut[(w[j >> 2] >> ((j & 3) * 8)) & 255u];
    } else {
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const int sxc = s0 + j;
        if (sxc >= 0 && sxc < cw3) v[j] = lut[src[sxc]];
      }
    }
  }
  // (the store tail is frame_yuv_to_tiles_kernel's too, each in its own text: behind a shared __device__ function both kernels' branch layout changes)
  float* d = p.dst + r * row + xc0;
  if (xc0 + 12 <= row && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<float4*>(d)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (xc0 + j < row) d[j] = v[j];
  }
}

// ---- Y'CbCr 4:2:0 frames (the arithmetic: include/film_hip.h, "The 4:2:0 arithmetic" and "The 10-bit 4:2:0 arithmetic") ---------------
// The twelve floats every 4:2:0 kernel's constants end with: the nine coefficients of a colour matrix, computed on the HOST in double from
// (Kr, Kb) and rounded to float32 once, and the two scales and the offset of the way out (those of the depth: 219 / 16 / 224 or 876 / 64 / 896).
struct YuvMatrix {
  float a_r, a_b, g_b, g_r;              // in: R = y + a_r cr, B = y + a_b cb, G = (y - g_b cb) - g_r cr
  float kr, kg, kb, s_b, s_r;            // out: Yf = (kr R + kg G) + kb B, cbf = (B - Yf) s_b, crf = (R - Yf) s_r
  float y_scale, y_off, c_scale;         // out: Y = q(Yf y_scale + y_off), C = q(m c_scale + mid)
};
// 8 bits: the luma and chroma value of every byte, divided on the HOST with IEEE division.  Passed by value (2 KB of kernel arguments).
struct YuvTables {
  float y[256], c[256];
  YuvMatrix m;
};
// 10 bits: y = (float(v) - y_sub) / y_div, c = (float(v) - 512) / c_div.  The two 1024-entry tables of quotients would be 8 KB - more than a kernel's argument block holds - so there are none: the cut DIVIDES on the device,
// (float(v) - sub) / div with the divisor a kernel argument.  hipcc's fp32 division is correctly rounded by default
// (-fhip-fp32-correctly-rounded-divide-sqrt: the v_div_scale / v_div_fmas / v_div_fixup sequence) and this library is built without
// fast-math and without contraction, so the quotient has the bits of the host's IEEE division; no quotient here is subnormal.  Chosen over
// device-resident tables copied into LDS by every workgroup: no per-device allocation for launchers that have no handle to own it, no
// 8 KB LDS fill per workgroup for ten look-ups per thread, and nothing an input word could index.
struct Yuv10Consts {
  float y_sub, y_div, c_div;
  YuvMatrix m;
};
const YuvTables& yuv_tables(int pix);   // ("host", below)
Yuv10Consts yuv10_consts(int pix);

// n <= 4 16-bit samples from p (2-byte aligned) as the low words of a 64-bit value, read as the one, two or three ALIGNED 32-bit words
// that hold them: every word read holds at least one of the samples asked for
__device__ __forceinline__ uint64_t load_samples_aligned(const uint16_t* p, int n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
  const unsigned off = (unsigned)(a >> 1) & 1u;   // samples in front of p in its word
  uint64_t v = wp[0];
  if (off + (unsigned)n > 2) v |= (uint64_t)wp[1] << 32;
  if (off) {
    v >>= 16;
    if ((unsigned)n > 3) v |= (uint64_t)wp[2] << 48;
  }
  return v;
}

// What a Y'CbCr layout decides, for the one cut and the one quantiser below.  A frame is its Y plane [H][W] first, then Cb [H >> SY][W >> SX]
// and Cr [H >> SY][W >> SX] (planar) or, 4:2:0 only, CbCr [H/2][W/2][2] (NV12, P010): H * W * 3 / 2 samples (4:2:0; H, W even), 2 H W (4:2:2;
// W even) or 3 H W (4:4:4; any H, W).  A sample is a byte, or a little-endian 16-bit word that keeps its 10-bit code in bits 0-9 (I010, I210,
// I410: the upper six are ignored) or in bits 6-15 (P010: the lower six are).
template <int LAYOUT> struct YuvLayout {
  static_assert(LAYOUT == FILM_PIX_I420 || LAYOUT == FILM_PIX_NV12 || LAYOUT == FILM_PIX_I010 || LAYOUT == FILM_PIX_P010 || LAYOUT == FILM_PIX_I422 ||
                LAYOUT == FILM_PIX_I444 || LAYOUT == FILM_PIX_I210 || LAYOUT == FILM_PIX_I410, "a Y'CbCr layout");
  static constexpr int PIX = LAYOUT;
  static constexpr bool WIDE = LAYOUT == FILM_PIX_I010 || LAYOUT == FILM_PIX_P010 || LAYOUT == FILM_PIX_I210 || LAYOUT == FILM_PIX_I410;   // 10-bit codes in 16-bit samples
  static constexpr bool SEMI_PLANAR = LAYOUT == FILM_PIX_NV12 || LAYOUT == FILM_PIX_P010;
  static constexpr int SX = LAYOUT == FILM_PIX_I444 || LAYOUT == FILM_PIX_I410 ? 0 : 1;            // chroma column of frame column x: x >> SX
  static constexpr int SY = SX == 0 || LAYOUT == FILM_PIX_I422 || LAYOUT == FILM_PIX_I210 ? 0 : 1;   // chroma row of frame row y: y >> SY
  static constexpr int GROUP_CHROMA = SX ? 3 : 4;   // the most chroma samples per plane under four pixels of a row
  // samples of one chroma plane of an H x W frame (H * W = plane)
  static __host__ __device__ __forceinline__ int64_t chroma_plane(int64_t plane) { return SX + SY == 2 ? plane / 4 : SX + SY == 1 ? plane / 2 : plane; }
  using Sample = std::conditional_t<WIDE, uint16_t, uint8_t>;
  using Consts = std::conditional_t<WIDE, Yuv10Consts, YuvTables>;       // the kernels' constants
  static constexpr int BITS = 8 * (int)sizeof(Sample), PER_WORD = 32 / BITS;   // of a stored sample; samples per 32-bit word
  static constexpr uint32_t MASK = (1u << BITS) - 1;
  static constexpr int SHIFT = LAYOUT == FILM_PIX_P010 ? 6 : 0;          // where the code sits in the sample; what the quantiser shifts by
  static constexpr int QMAX = WIDE ? 1023 : 255, MID = WIDE ? 512 : 128;  // the largest code, the chroma midpoint
  static __device__ __forceinline__ uint32_t code(uint32_t w) { return ((w & MASK) >> SHIFT) & (uint32_t)QMAX; }
  // n samples from p as the low samples of a 64-bit value, read as the aligned 32-bit words that hold them
  static __device__ __forceinline__ uint64_t load(const Sample* p, int n) {
    if constexpr (WIDE) return load_samples_aligned(p, n);
    else return load_bytes_aligned(p, n);
  }
  static Consts consts(int pix) {
    if constexpr (WIDE) return yuv10_consts(pix);
    else return yuv_tables(pix);
  }
};

// frame_u8_to_tiles_kernel on a Y'CbCr frame batch: p.src points at samples (4-byte aligned), frame b at sample b * S, S the samples of a frame
// (a 4:4:4 frame of odd size: not a word boundary - every read below is of the aligned words that hold a sample).
// thread = four pixels (twelve floats) of one row of the tile buffer.  Pixel (fy, fx) of the FRAME takes the chroma sample (fy >> SY, fx >> SX):
// origins and patch sizes may be odd, so the pairing follows the frame coordinate.  A group wholly inside the tile's content reads its four
// Y samples and its two or three (4:4:4: four) chroma samples per plane as aligned 32-bit words (YuvLayout::load), P010 as the two or three aligned
// words that ARE its CbCr pairs (a pair never straddles a word, W being even); a group that touches the padding or the row's end goes sample by sample.
// 8 bits look the luma and chroma values up in the two tables (copied to LDS); 10 bits divide (Yuv10Consts) and declare no LDS.
template <bool OVERLAP, int LAYOUT>
__global__ __launch_bounds__(256) void frame_yuv_to_tiles_kernel(TileMapParams p, typename YuvLayout<LAYOUT>::Consts k) {
  using L = YuvLayout<LAYOUT>;
  using Sample = typename L::Sample;
  const float *ly = nullptr, *lc = nullptr;
  if constexpr (!L::WIDE) {
    __shared__ float lut_y[256], lut_c[256];
    lut_y[threadIdx.x] = k.y[threadIdx.x];
    lut_c[threadIdx.x] = k.c[threadIdx.x];
    __syncthreads();
    ly = lut_y; lc = lut_c;
  }
  const int row = p.TW * 3;
  const int groups = (p.TW + 3) / 4;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)p.ntiles * p.TH * groups) return;
  const int xp0 = (int)(g % groups) * 4;      // first pixel of the group in the tile row
  const int64_t r = g / groups;               // row of the tile buffer
  using C = TileContent<OVERLAP>;
  int y, b, ty, tx;
  tile_row(p, r, y, b, ty, tx);
  const int ch = C::rows(p), cw = C::cols(p);                         // the tile's content: rows, pixels per row
  const int sy = y - p.oy, s0 = xp0 - p.ox;                           // content row, content pixel of the group's first pixel
  float v[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) v[j] = 0.f;   // tf.image.pad_to_bounding_box pads with zeros
  if (sy >= 0 && sy < ch && s0 + 4 > 0 && s0 < cw) {
    const int fy = C::row0(p, ty) + sy;
    const int fx = C::col0(p, tx) + s0;   // frame column of the group's first pixel
    const int64_t plane = (int64_t)p.H * p.W;
    const int64_t cplane = L::chroma_plane(plane);
    const Sample* frame0 = reinterpret_cast<const Sample*>(p.src) + (int64_t)b * (plane + 2 * cplane);
    const Sample* yrow = frame0 + (int64_t)fy * p.W;
    const int hw = p.W >> L::SX;
    // semi-planar: one row of Cb Cr pairs; planar: a Cb row and, one chroma plane further on, the Cr row
    const Sample* crow = frame0 + plane + (int64_t)(fy >> L::SY) * (L::SEMI_PLANAR ? p.W : hw);
    const int64_t cr_off = L::SEMI_PLANAR ? 1 : cplane;
    uint32_t yb[4], cbb[4], crb[4];
    bool have[4];
    if (s0 >= 0 && s0 + 4 <= cw) {
      const uint64_t yw = L::load(yrow + fx, 4);
      const int c0 = fx >> L::SX, nc = ((fx + 3) >> L::SX) - c0 + 1;      // two chroma samples per plane, three from an odd column; 4:4:4: four
      uint32_t cbs[L::GROUP_CHROMA], crs[L::GROUP_CHROMA];
      if constexpr (LAYOUT == FILM_PIX_P010) {
        const uint32_t* cwp = reinterpret_cast<const uint32_t*>(crow) + c0;   // (4-byte aligned: the frame is, and H * W and W are even)
        const uint32_t w0 = cwp[0], w1 = cwp[1], w2 = nc > 2 ? cwp[2] : 0u;
        cbs[0] = w0 & 0xffffu; crs[0] = w0 >> 16;
        cbs[1] = w1 & 0xffffu; crs[1] = w1 >> 16;
        cbs[2] = w2 & 0xffffu; crs[2] = w2 >> 16;
      } else if constexpr (L::SEMI_PLANAR) {
        const uint64_t w = L::load(crow + 2 * c0, 2 * nc);
#pragma unroll
        for (int q = 0; q < 3; ++q) { cbs[q] = (uint32_t)(w >> (2 * L::BITS * q)) & L::MASK; crs[q] = (uint32_t)(w >> (2 * L::BITS * q + L::BITS)) & L::MASK; }
      } else {
        const uint64_t wb = L::load(crow + c0, nc), wr = L::load(crow + cr_off + c0, nc);
#pragma unroll
        for (int q = 0; q < L::GROUP_CHROMA; ++q) { cbs[q] = (uint32_t)(wb >> (L::BITS * q)) & L::MASK; crs[q] = (uint32_t)(wr >> (L::BITS * q)) & L::MASK; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        yb[j] = (uint32_t)(yw >> (L::BITS * j)) & L::MASK;
        if constexpr (L::SX == 0) {
          cbb[j] = cbs[j]; crb[j] = crs[j];
        } else {
          const int q = ((fx + j) >> 1) - c0;
          cbb[j] = q == 0 ? cbs[0] : q == 1 ? cbs[1] : cbs[2];
          crb[j] = q == 0 ? crs[0] : q == 1 ? crs[1] : crs[2];
        }
        have[j] = true;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        have[j] = s0 + j >= 0 && s0 + j < cw;
        yb[j] = cbb[j] = crb[j] = 0;
        if (have[j]) {
          const int c = (fx + j) >> L::SX;
          yb[j] = yrow[fx + j];
          cbb[j] = L::SEMI_PLANAR ? crow[2 * c] : crow[c];
          crb[j] = L::SEMI_PLANAR ? crow[2 * c + 1] : crow[cr_off + c];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!have[j]) continue;
      float yv, cb, cr;
      if constexpr (L::WIDE) {
        yv = ((float)L::code(yb[j]) - k.y_sub) / k.y_div;
        cb = ((float)L::code(cbb[j]) - (float)L::MID) / k.c_div; cr = ((float)L::code(crb[j]) - (float)L::MID) / k.c_div;
      } else {
        yv = ly[yb[j]]; cb = lc[cbb[j]]; cr = lc[crb[j]];
      }
      v[3 * j] = clip01(yv + k.m.a_r * cr);
      v[3 * j + 1] = clip01((yv - k.m.g_b * cb) - k.m.g_r * cr);
      v[3 * j + 2] = clip01(yv + k.m.a_b * cb);
    }
  }
  const int xc0 = xp0 * 3;
  float* d = p.dst + r * row + xc0;
  if (xc0 + 12 <= row && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<float4*>(d)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (xc0 + j < row) d[j] = v[j];
  }   // (own text: see frame_u8_to_tiles_kernel)
}

// ---- the two ways out to 8 bits ---------------------------------------------------------------------------------------------------
// eval/util.py:51-52 (write_image): clip(x * 255, 0, 255) + 0.5, truncated to uint8 - the same float32 operations in the same order
// (no fused multiply-add: the file is built with -ffp-contract=off), four values per thread
__global__ __launch_bounds__(256) void to_uint8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 3 < n && ((reinterpret_cast<uintptr_t>(src + i) & 15) == 0) && ((reinterpret_cast<uintptr_t>(dst + i) & 3) == 0)) {
    const float4 v = *reinterpret_cast<const float4*>(src + i);
    *reinterpret_cast<uint32_t*>(dst + i) = quantise<255>(v.x * 255.f) | (quantise<255>(v.y * 255.f) << 8) | (quantise<255>(v.z * 255.f) << 16) | (quantise<255>(v.w * 255.f) << 24);
  } else {
    for (int64_t k = i; k < n && k < i + 4; ++k) dst[k] = (uint8_t)quantise<255>(src[k] * 255.f);
  }
}

// N quantised samples of PER_WORD = 4 (bytes) or 2 (16-bit) to a 32-bit word, in memory order, as the N / PER_WORD whole words at d (4-byte aligned)
template <int PER_WORD, int N>
__device__ __forceinline__ void store_sample_words(void* d, const uint32_t (&q)[N]) {
#pragma unroll
  for (int w = 0; w < N / PER_WORD; ++w) {
    uint32_t word = q[w * PER_WORD];
#pragma unroll
    for (int i = 1; i < PER_WORD; ++i) word |= q[w * PER_WORD + i] << (i * (32 / PER_WORD));
    reinterpret_cast<uint32_t*>(d)[w] = word;
  }
}

// float32 frame [H][W][3] -> the planes of one Y'CbCr frame (film_to_yuv / film_to_yuv420; the quantisation of a Y'CbCr stream's push): dst points
// at samples (10 bits: 2-byte aligned).  thread = 2 rows x 8 pixels: sixteen Y samples and, per plane, four chroma samples (4:2:0: the 2 x 2 means),
// two rows of four (4:2:2: the 1 x 2 means) or two rows of eight (4:4:4: no mean), which leave as whole 32-bit words where the block is complete
// and the address allows, sample by sample otherwise.  A sample is the code << YuvLayout::SHIFT: the bits a 10-bit layout ignores are written as
// zero.  4:2:0: H and W are even; 4:2:2: W is even, an odd H ends on a block of one row; 4:4:4: the last block of a row may hold an odd count of pixels.
template <int LAYOUT>
__global__ __launch_bounds__(256) void rgb_to_yuv_kernel(const float* __restrict__ src, typename YuvLayout<LAYOUT>::Sample* __restrict__ dst, int H, int W,
                                                         typename YuvLayout<LAYOUT>::Consts k) {
  using L = YuvLayout<LAYOUT>;
  using Sample = typename L::Sample;
  constexpr int CR = L::SY ? 1 : 2, CN = L::SX ? 4 : 8;   // chroma rows of a block, chroma samples per row and plane
  const int bpr = (W + 7) / 8;      // blocks per row pair
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)((H + 1) / 2) * bpr) return;
  const int x0 = (int)(i % bpr) * 8, y0 = (int)(i / bpr) * 2;
  const int np = min(8, W - x0);    // pixels of the block per row: even, but for 4:4:4
  const int rows = L::SY ? 2 : min(2, H - y0);   // rows of the block: one at the end of an odd H (which only SY = 0 has)
  uint32_t yq[2][8], cbq[CR][CN], crq[CR][CN];
  float cbf[2][8], crf[2][8];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    if (dy >= rows) continue;
    const float* s = src + ((int64_t)(y0 + dy) * W + x0) * 3;
    float px[24];
    if (np == 8 && (reinterpret_cast<uintptr_t>(s) & 15) == 0) {
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const float4 f = reinterpret_cast<const float4*>(s)[q];
        px[4 * q] = f.x; px[4 * q + 1] = f.y; px[4 * q + 2] = f.z; px[4 * q + 3] = f.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 24; ++q) px[q] = q < np * 3 ? s[q] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float R = clip01(px[3 * j]), G = clip01(px[3 * j + 1]), B = clip01(px[3 * j + 2]);
      const float Yf = (k.m.kr * R + k.m.kg * G) + k.m.kb * B;
      cbf[dy][j] = (B - Yf) * k.m.s_b;
      crf[dy][j] = (R - Yf) * k.m.s_r;
      yq[dy][j] = quantise<L::QMAX>(Yf * k.m.y_scale + k.m.y_off) << L::SHIFT;
    }
  }
#pragma unroll
  for (int c = 0; c < CR; ++c) {
    if (c >= rows) continue;
#pragma unroll
    for (int q = 0; q < CN; ++q) {
      float mb, mr;
      if constexpr (L::SY) {          // 4:2:0: the 2 x 2 box
        mb = ((cbf[0][2 * q] + cbf[0][2 * q + 1]) + (cbf[1][2 * q] + cbf[1][2 * q + 1])) * 0.25f;
        mr = ((crf[0][2 * q] + crf[0][2 * q + 1]) + (crf[1][2 * q] + crf[1][2 * q + 1])) * 0.25f;
      } else if constexpr (L::SX) {   // 4:2:2: the pair of a row
        mb = (cbf[c][2 * q] + cbf[c][2 * q + 1]) * 0.5f;
        mr = (crf[c][2 * q] + crf[c][2 * q + 1]) * 0.5f;
      } else {                        // 4:4:4: the pixel's own
        mb = cbf[c][q];
        mr = crf[c][q];
      }
      cbq[c][q] = quantise<L::QMAX>(mb * k.m.c_scale + (float)L::MID) << L::SHIFT;
      crq[c][q] = quantise<L::QMAX>(mr * k.m.c_scale + (float)L::MID) << L::SHIFT;
    }
  }
  const int64_t plane = (int64_t)H * W;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    if (dy >= rows) continue;
    Sample* d = dst + (int64_t)(y0 + dy) * W + x0;
    if (np == 8 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
      store_sample_words<L::PER_WORD>(d, yq[dy]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < np) d[j] = (Sample)yq[dy][j];
    }
  }
  if constexpr (L::SEMI_PLANAR) {
    Sample* d = dst + plane + (int64_t)(y0 >> 1) * W + x0;
    if (np == 8 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
      const uint32_t pairs[8] = {cbq[0][0], crq[0][0], cbq[0][1], crq[0][1], cbq[0][2], crq[0][2], cbq[0][3], crq[0][3]};
      store_sample_words<L::PER_WORD>(d, pairs);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (2 * q < np) { d[2 * q] = (Sample)cbq[0][q]; d[2 * q + 1] = (Sample)crq[0][q]; }
    }
  } else {
    const int64_t cplane = L::chroma_plane(plane);
#pragma unroll
    for (int c = 0; c < CR; ++c) {
      if (c >= rows) continue;
      Sample* db = dst + plane + (int64_t)((y0 >> L::SY) + c) * (W >> L::SX) + (x0 >> L::SX);
      Sample* dr = db + cplane;
      if (np == 8 && (reinterpret_cast<uintptr_t>(db) & 3) == 0 && (reinterpret_cast<uintptr_t>(dr) & 3) == 0) {
        store_sample_words<L::PER_WORD>(db, cbq[c]);
        store_sample_words<L::PER_WORD>(dr, crq[c]);
      } else {
#pragma unroll
        for (int q = 0; q < CN; ++q)
          if ((q << L::SX) < np) { db[q] = (Sample)cbq[c][q]; dr[q] = (Sample)crq[c][q]; }
      }
    }
  }
}

// ---- overlapped tiles: every tile carries ovy / ovx pixels of its neighbours, the results are cross-faded ------------------
// Cross-fade weight (before normalisation) of tile i of an axis at frame position y: the distance to the nearest INTERIOR edge of
// the tile, counted from 1; an edge on the frame's border does not limit it; 0 outside the tile.  *s = the tile's origin.
__device__ __forceinline__ float fade_weight(int i, int y, int nb, int p, int o, int n, int e, int* s) {
  if (i < 0 || i >= nb) return 0.f;
  *s = film_tile_origin(i, p, o, n, e);
  if (y < *s || y >= *s + e) return 0.f;
  int a = 1 << 30;
  if (*s > 0) a = min(a, y - *s + 1);
  if (*s + e < n) a = min(a, *s + e - y);
  return (float)a;
}

// thread = one float of rows [y0, y0 + ny) of frames [b0, b0 + nfr).  A pixel of block (ky, kx) is covered by tiles of the block
// rows ky - 1 .. ky + 1 and columns kx - 1 .. kx + 1 only (2 * overlap <= patch).  Over the covering tiles in row-major order:
// acc = (wy * wx) * v for the first, acc = acc + (wy * wx) * v for the others, wy = a_i(y) / sum_i a_i(y) (one float32 operation
// each, no fma: this file is built with -ffp-contract=off).  Covering tiles below tile0 were added by an earlier launch - the sum
// goes on from dst; tiles from tile0 + ntiles on are left to a later one.
__global__ __launch_bounds__(256) void blend_tiles_kernel(TileMapParams p, int b0, int nfr, int y0, int ny) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int row = p.W * 3;
  if (i >= (int64_t)nfr * ny * row) return;
  const int xc = (int)(i % row);
  const int64_t r = i / row;
  const int y = y0 + (int)(r % ny);
  const int b = b0 + (int)(r / ny);
  const int x = xc / 3, c = xc - 3 * x;
  const int ky = y / p.ph, kx = x / p.pw;
  float ay[3], ax[3];
  int sy[3] = {0, 0, 0}, sx[3] = {0, 0, 0};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ay[d] = fade_weight(ky - 1 + d, y, p.bh, p.ph, p.ovy, p.H, p.eh, &sy[d]);
    ax[d] = fade_weight(kx - 1 + d, x, p.bw, p.pw, p.ovx, p.W, p.ew, &sx[d]);
  }
  const float sum_y = (ay[0] + ay[1]) + ay[2], sum_x = (ax[0] + ax[1]) + ax[2];   // (integers below 2^31: exact)
  const int64_t o = (((int64_t)b * p.H + y) * p.W) * 3 + xc;
  const int first = b * p.bh * p.bw;
  float acc = 0.f;
  bool have = false, mine = false;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    if (ay[dy] == 0.f) continue;
    const float wy = ay[dy] / sum_y;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      if (ax[dx] == 0.f) continue;
      const int n = first + (ky - 1 + dy) * p.bw + (kx - 1 + dx);
      if (n >= p.tile0 + p.ntiles) continue;
      if (n < p.tile0) {
        if (!have) { acc = p.dst[o]; have = true; }
        continue;
      }
      const float w = wy * (ax[dx] / sum_x);
      const float v = p.src[(((int64_t)(n - p.tile0) * p.TH + p.oy + (y - sy[dy])) * p.TW + p.ox + (x - sx[dx])) * 3 + c];
      const float t = w * v;
      acc = have ? acc + t : t;
      have = true; mine = true;
    }
  }
  if (mine) p.dst[o] = acc;
}

// ---- the per-frame sample histogram (film_frame_histogram; include/film_hip.h, "Scene cuts") ----------------------------------------------
// hist[p][v] += the samples of plane p with 8-bit code v, over the n elements of one frame: bytes (LAYOUT = FILM_PIX_U8 / I420 / NV12) or
// floats (FILM_PIX_F32, whose code is film_to_uint8's byte).  `plane` = H * W, the samples of the Y plane of a Y'CbCr frame, `cplane` those of
// one of its chroma planes (H * W / 4, H * W / 2 or H * W: the planar instances serve every subsampling; the I422 / I444 frames run the I420
// instance, I210 / I410 the I010 one).
//   loads     The frame is walked in the ALIGNED 16-byte vectors that hold it, one vector per lane and step of a grid-stride loop: a
//             vector that lies wholly inside the frame is one 16-byte load; the first vector of a frame that does not start on a 16-byte
//             boundary and the last partial one are read as the 32-bit words that hold at least one element of the frame (the pointer is
//             4-byte aligned, so only the last word can be partial: the allocation-in-whole-words contract of the 8-bit cuts), and count
//             only the elements of the frame.
//   planes    interleaved RGB: element index mod 3; I420: three consecutive ranges; NV12: the Y range, then Cb at even and Cr at odd offsets.
//   10 bits   LAYOUT = FILM_PIX_I010 / P010: the elements are 16-bit samples, eight per vector and two per word (n and `plane` count samples;
//             the pointer is 4-byte aligned; a 4:4:4 frame of odd size has an odd n: its last word is partial and, like every word of a
//             vector that is not whole, is counted by element); planes as I420 / NV12; a sample counts in bin code >> 2,
//             the code being bits 0-9 (I010) or 6-15 (P010) of the word.
//   counting  LDS integer atomics into HIST_COPIES sub-histograms per workgroup, laid out [bin][copy] with copy = lane & 7: eight
//             neighbouring lanes never share an address, a flat picture (every lane on one bin) meets 8-way instead of 64-way same-address
//             serialisation, and the copies of a bin lie in eight consecutive banks.
//   flush     a workgroup adds its non-zero bins to the 768 global counters with integer atomicAdd: the sums do not depend on the grid or
//             the arrival order.  hist is zeroed by the launcher.
constexpr int HIST_COPIES = 8;
template <int LAYOUT>
__global__ __launch_bounds__(FILM_HIST_THREADS) void frame_histogram_kernel(const void* __restrict__ frame, int64_t n, int64_t plane, int64_t cplane,
                                                                            uint32_t* __restrict__ hist) {
  constexpr bool F32 = LAYOUT == FILM_PIX_F32;
  constexpr bool U16 = LAYOUT == FILM_PIX_I010 || LAYOUT == FILM_PIX_P010;   // 10-bit samples in 16-bit words: the code counted is v >> 2
  constexpr int EPV = F32 ? 4 : U16 ? 8 : 16;   // elements per 16-byte vector
  constexpr int EPW = EPV / 4;        // ... per 32-bit word
  __shared__ uint32_t sub[FILM_HIST_BINS * HIST_COPIES];
  for (int i = threadIdx.x; i < FILM_HIST_BINS * HIST_COPIES; i += FILM_HIST_THREADS) sub[i] = 0;
  __syncthreads();
  const uintptr_t a = reinterpret_cast<uintptr_t>(frame);
  const uint4* base = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(frame) - (a & 15));   // (pointer arithmetic: the loads stay global loads)
  const int head = (int)(a & 15) / (F32 ? 4 : U16 ? 2 : 1);   // elements of vector 0 in front of the frame
  const int64_t nvec = (head + n + EPV - 1) / EPV;
  const int copy = threadIdx.x & (HIST_COPIES - 1);
  for (int64_t v = (int64_t)blockIdx.x * FILM_HIST_THREADS + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * FILM_HIST_THREADS) {
    const int64_t e0 = v * EPV - head;   // the frame element at position 0 of the vector (negative in the head)
    const bool whole = e0 >= 0 && e0 + EPV <= n;
    uint32_t w[4];
    if (whole) {
      const uint4 q = base[v];
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
      const uint32_t* wp = reinterpret_cast<const uint32_t*>(base + v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t ek = e0 + k * EPW;   // word k holds elements [ek, ek + EPW)
        w[k] = (ek + EPW > 0 && ek < n) ? wp[k] : 0u;
      }
    }
    // what decides the plane of position j, as small integers
    const int c0 = (int)(((uint32_t)v % 3u + (uint32_t)(18 - head)) % 3u);           // RGB: channel of position 0 = (EPV v - head) mod 3, EPV mod 3 = 1 (v < 2^29)
    const int d1 = (int)min((int64_t)EPV, max((int64_t)0, plane - e0));              // Y'CbCr: positions below d1 are Y ...
    const int d2 = (int)min((int64_t)EPV, max((int64_t)0, plane + cplane - e0));     // ... planar: below d2 Cb, from d2 on Cr
    const int par = (int)((e0 - plane) & 1);                                         // NV12: parity of position 0 inside the CbCr plane
#pragma unroll
    for (int j = 0; j < EPV; ++j) {
      if (!whole && (e0 + j < 0 || e0 + j >= n)) continue;
      uint32_t code;
      if (F32) code = quantise<255>(__uint_as_float(w[j]) * 255.f) & 255u;  // film_to_uint8's operations (& 255: a NaN stays inside the bins)
      else if (LAYOUT == FILM_PIX_I010) code = (w[j / 2] >> ((j & 1) * 16 + 2)) & 255u;    // (w & 1023) >> 2
      else if (LAYOUT == FILM_PIX_P010) code = (w[j / 2] >> ((j & 1) * 16 + 8)) & 255u;    // (w >> 6) >> 2
      else code = (w[j / 4] >> ((j & 3) * 8)) & 255u;
      int p;
      if (LAYOUT == FILM_PIX_I420 || LAYOUT == FILM_PIX_I010) p = (j >= d1) + (j >= d2);
      else if (LAYOUT == FILM_PIX_NV12 || LAYOUT == FILM_PIX_P010) p = j < d1 ? 0 : 1 + ((par + j) & 1);
      else { p = c0 + j % 3; p = p >= 3 ? p - 3 : p; }
      atomicAdd(&sub[(p * 256 + (int)code) * HIST_COPIES + copy], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < FILM_HIST_BINS; b += FILM_HIST_THREADS) {
    uint32_t sum = 0;
#pragma unroll
    for (int c = 0; c < HIST_COPIES; ++c) sum += sub[b * HIST_COPIES + c];
    if (sum) atomicAdd(&hist[b], sum);
  }
}

// ---- the block SADs of two frames (film_frame_diff; include/film_hip.h, "Duplicate frames") ------------------------------------------------
// out[p] = {total, max, over, blocks} of the 8 x 8 block SADs of plane p between frames a and b, on full-depth codes.  Integers only (the F32
// quantisation aside), so the result does not depend on the grid or the arrival order.
//   groups    A frame is one to three GROUPS of planes whose samples interleave: a planar Y'CbCr frame is three groups of one plane, a
//             semi-planar one is Y and the CbCr pairs (two planes), an RGB frame is one group of three.  A group of NP planes of hp x wp
//             samples is hp rows of wp * NP elements; its blocks are those of its planes, anchored on the plane.
//   lanes     one lane per block position of a group - NP blocks -, adjacent lanes on adjacent blocks of a block row, in a grid-stride loop
//             per group (the group is a compile-time value inside the loop, so the NP block SADs stay in registers and no accumulator is
//             indexed by a runtime plane).  A whole row segment - eight samples per plane - whose address is 4-byte aligned is read as the
//             2 NP (8-bit) or 4 NP (16-bit) 32-bit words that ARE it: wave-wide that is one coalesced run of 8 or 16 bytes per lane, and
//             v_sad_u8 / v_sad_u16 take the words as they are (interleaved planes: masked per plane first - a masked-out byte adds 0).  A
//             partial block or an unaligned row goes sample by sample.  No load reaches outside the frame.
//   codes     8 bits: the byte; 10 bits: (w >> SHIFT) & 1023, on both halves of a word at once; F32: film_to_uint8's byte, as the histogram.
//   reduce    per lane 3 x {total (64-bit), max, over, blocks}; wave shuffles, LDS across the four waves, then one lane per plane flushes
//             with integer atomics (64-bit add, unsigned max, add, add).  `blocks` counts the blocks the lanes VISITED.  out is zeroed by the launcher.
struct DiffGroup { int64_t off; int hp, wp, bw; int64_t units; };   // first element, plane size in samples, blocks per block row, block positions
struct DiffParams {
  const void *a, *b;
  DiffGroup g[3];
  uint32_t lo;
  unsigned long long* out;
};
// what the comparison asks of a layout: the two RGB types, else what YuvLayout<LAYOUT> says (sample width, semi-planar chroma, where the code sits)
struct RgbDiffTraits { static constexpr bool WIDE = false, SEMI_PLANAR = false; static constexpr int SHIFT = 0; };
template <int LAYOUT> struct DiffLayout {
  static constexpr bool F32 = LAYOUT == FILM_PIX_F32, RGB = F32 || LAYOUT == FILM_PIX_U8;
  using L = std::conditional_t<RGB, RgbDiffTraits, YuvLayout<RGB ? FILM_PIX_I420 : LAYOUT>>;
  static constexpr bool WIDE = L::WIDE, SEMI = L::SEMI_PLANAR;
  static constexpr int SHIFT = L::SHIFT;
  static constexpr int GROUPS = RGB ? 1 : SEMI ? 2 : 3;
  static constexpr int planes(int g) { return RGB ? 3 : SEMI && g == 1 ? 2 : 1; }          // NP of group g
  static constexpr int plane(int g, int c) { return RGB ? c : SEMI ? (g ? 1 + c : 0) : g; }   // the plane of its component c
  using Elem = std::conditional_t<F32, float, std::conditional_t<WIDE, uint16_t, uint8_t>>;
};
// byte t of word k of a row segment of three interleaved 8-bit planes belongs to plane (4 k + t) % 3
constexpr uint32_t rgb_word_mask(int k, int c) {
  uint32_t m = 0;
  for (int t = 0; t < 4; ++t)
    if ((4 * k + t) % 3 == c) m |= 0xffu << (8 * t);
  return m;
}
// s[c] += the absolute differences of component c over `cols` samples per plane of one row of a block
template <int LAYOUT, int NP>
__device__ __forceinline__ void diff_row(const typename DiffLayout<LAYOUT>::Elem* pa, const typename DiffLayout<LAYOUT>::Elem* pb, int cols, uint32_t (&s)[NP]) {
  using D = DiffLayout<LAYOUT>;
  if constexpr (D::F32) {
    auto q = [](float x) { return (int)(quantise<255>(x * 255.f) & 255u); };   // film_to_uint8's operations, as frame_histogram_kernel's
    if (cols == 8) {
#pragma unroll
      for (int e = 0; e < 8 * NP; ++e) s[e % NP] += (uint32_t)abs(q(pa[e]) - q(pb[e]));
    } else {
      for (int x = 0; x < cols; ++x)
#pragma unroll
        for (int c = 0; c < NP; ++c) s[c] += (uint32_t)abs(q(pa[x * NP + c]) - q(pb[x * NP + c]));
    }
  } else {
    const bool words = cols == 8 && ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 3) == 0;
    if (words) {
      const uint32_t* wa = reinterpret_cast<const uint32_t*>(pa);
      const uint32_t* wb = reinterpret_cast<const uint32_t*>(pb);
      constexpr int NW = 8 * NP * (int)sizeof(typename D::Elem) / 4;
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        uint32_t x = wa[k], y = wb[k];
        if constexpr (D::WIDE) {
          x = (x >> D::SHIFT) & 0x03ff03ffu; y = (y >> D::SHIFT) & 0x03ff03ffu;   // both codes of the word
          if constexpr (NP == 1) s[0] = __builtin_amdgcn_sad_u16(x, y, s[0]);
          else {   // a CbCr pair
            s[0] = __builtin_amdgcn_sad_u16(x & 0xffffu, y & 0xffffu, s[0]);
            s[1] = __builtin_amdgcn_sad_u16(x >> 16, y >> 16, s[1]);
          }
        } else if constexpr (NP == 1) s[0] = __builtin_amdgcn_sad_u8(x, y, s[0]);
        else if constexpr (NP == 2) {
          s[0] = __builtin_amdgcn_sad_u8(x & 0x00ff00ffu, y & 0x00ff00ffu, s[0]);
          s[1] = __builtin_amdgcn_sad_u8(x & 0xff00ff00u, y & 0xff00ff00u, s[1]);
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] = __builtin_amdgcn_sad_u8(x & rgb_word_mask(k % 3, c), y & rgb_word_mask(k % 3, c), s[c]);
        }
      }
    } else {
      for (int x = 0; x < cols; ++x)
#pragma unroll
        for (int c = 0; c < NP; ++c) {
          int u = pa[x * NP + c], v = pb[x * NP + c];
          if constexpr (D::WIDE) { u = (u >> D::SHIFT) & 1023; v = (v >> D::SHIFT) & 1023; }
          s[c] += (uint32_t)abs(u - v);
        }
    }
  }
}
struct DiffAcc { unsigned long long total[3]; uint32_t max[3], over[3], blocks[3]; };
template <int LAYOUT, int G>
__device__ __forceinline__ void diff_group(const DiffParams& p, DiffAcc& acc) {
  using D = DiffLayout<LAYOUT>;
  using Elem = typename D::Elem;
  constexpr int NP = D::planes(G);
  const DiffGroup g = p.g[G];
  const int64_t pitch = (int64_t)g.wp * NP;
  for (int64_t u = (int64_t)blockIdx.x * FILM_DIFF_THREADS + threadIdx.x; u < g.units; u += (int64_t)gridDim.x * FILM_DIFF_THREADS) {
    const int i = (int)(u / g.bw), j = (int)(u % g.bw);
    const int rows = min(8, g.hp - 8 * i), cols = min(8, g.wp - 8 * j);
    const int64_t e0 = g.off + (int64_t)(8 * i) * pitch + (int64_t)(8 * j) * NP;
    const Elem* pa = static_cast<const Elem*>(p.a) + e0;
    const Elem* pb = static_cast<const Elem*>(p.b) + e0;
    uint32_t s[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) s[c] = 0;
    if (rows == 8) {
#pragma unroll
      for (int r = 0; r < 8; ++r) diff_row<LAYOUT, NP>(pa + r * pitch, pb + r * pitch, cols, s);
    } else {
      for (int r = 0; r < rows; ++r) diff_row<LAYOUT, NP>(pa + r * pitch, pb + r * pitch, cols, s);
    }
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      const int pl = D::plane(G, c);
      acc.total[pl] += s[c];
      acc.max[pl] = max(acc.max[pl], s[c]);
      acc.over[pl] += s[c] > p.lo ? 1u : 0u;
      acc.blocks[pl] += 1u;
    }
  }
}
template <int LAYOUT>
__global__ __launch_bounds__(FILM_DIFF_THREADS) void frame_diff_kernel(DiffParams p) {
  using D = DiffLayout<LAYOUT>;
  DiffAcc acc{};
  diff_group<LAYOUT, 0>(p, acc);
  if constexpr (D::GROUPS > 1) diff_group<LAYOUT, 1>(p, acc);
  if constexpr (D::GROUPS > 2) diff_group<LAYOUT, 2>(p, acc);
  // wave: shuffles; workgroup: LDS; device: one lane per plane
  constexpr int WAVES = FILM_DIFF_THREADS / 64;
  __shared__ unsigned long long sh_total[WAVES][3];
  __shared__ uint32_t sh_rest[WAVES][3][3];
#pragma unroll
  for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      acc.total[pl] += __shfl_down(acc.total[pl], d, 64);
      acc.max[pl] = max(acc.max[pl], (uint32_t)__shfl_down(acc.max[pl], d, 64));
      acc.over[pl] += __shfl_down(acc.over[pl], d, 64);
      acc.blocks[pl] += __shfl_down(acc.blocks[pl], d, 64);
    }
  }
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      sh_total[wave][pl] = acc.total[pl];
      sh_rest[wave][pl][0] = acc.max[pl]; sh_rest[wave][pl][1] = acc.over[pl]; sh_rest[wave][pl][2] = acc.blocks[pl];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int pl = threadIdx.x;
    unsigned long long total = 0, mx = 0, over = 0, blocks = 0;
    for (int w = 0; w < WAVES; ++w) {
      total += sh_total[w][pl];
      mx = max(mx, (unsigned long long)sh_rest[w][pl][0]);
      over += sh_rest[w][pl][1]; blocks += sh_rest[w][pl][2];
    }
    unsigned long long* o = p.out + 4 * pl;
    if (total) atomicAdd(o, total);
    if (mx) atomicMax(o + 1, mx);
    if (over) atomicAdd(o + 2, over);
    if (blocks) atomicAdd(o + 3, blocks);
  }
}

}  // namespace

// One frame's histogram: zeroes the 768 counters, then counts.  At most FILM_HIST_WG_PER_CU workgroups per compute unit, fewer for a frame
// that has fewer vectors; the grid-stride loop takes the rest.  (The launcher stands beside its kernel; launch_units: "host" below.)
hipError_t film_launch_frame_histogram(const void* frame, int H, int W, int pix, uint32_t* hist, hipStream_t s) {
  const int layout = pix_layout(pix);   // (the colour flags do not enter)
  const bool yuv = pix_is_yuv(pix);
  if (!frame || !hist || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31) || (reinterpret_cast<uintptr_t>(frame) & 3)) return hipErrorInvalidValue;
  if (layout != FILM_PIX_F32 && layout != FILM_PIX_U8 && !yuv) return hipErrorInvalidValue;
  const ChromaShift cs = pix_chroma_shift(pix);
  if (yuv && ((W & cs.sx) | (H & cs.sy))) return hipErrorInvalidValue;
  const int64_t plane = (int64_t)H * W, cplane = yuv ? (int64_t)(H >> cs.sy) * (W >> cs.sx) : 0, n = yuv ? plane + 2 * cplane : plane * 3;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess) e = hipMemsetAsync(hist, 0, FILM_HIST_BINS * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const int epv = FILM_HIST_VEC_BYTES / pix_sample_bytes(pix);
  const int64_t nvec = (n + epv - 1) / epv + 1;   // (+ 1: a frame that starts inside a vector)
  const int64_t grid = std::min<int64_t>((int64_t)std::max(cus, 1) * FILM_HIST_WG_PER_CU, (nvec + FILM_HIST_THREADS - 1) / FILM_HIST_THREADS);
  auto kernel = layout == FILM_PIX_F32 ? frame_histogram_kernel<FILM_PIX_F32> : layout == FILM_PIX_U8 ? frame_histogram_kernel<FILM_PIX_U8>
              : layout == FILM_PIX_NV12 ? frame_histogram_kernel<FILM_PIX_NV12> : layout == FILM_PIX_P010 ? frame_histogram_kernel<FILM_PIX_P010>
              : pix_is_yuv10(pix) ? frame_histogram_kernel<FILM_PIX_I010> : frame_histogram_kernel<FILM_PIX_I420>;   // (planar: every subsampling)
  static_assert(FILM_HIST_THREADS == 256, "launch_units starts workgroups of 256");
  return launch_units(kernel, grid * FILM_HIST_THREADS, s, frame, n, plane, cplane, hist);   // `grid` workgroups
}

// The block SADs of two frames: zeroes the twelve counters, then compares.  At most FILM_DIFF_WG_PER_CU workgroups per compute unit, fewer
// for a frame that has fewer block positions; the grid-stride loops take the rest.  The instances are the histogram's.
hipError_t film_launch_frame_diff(const void* a, const void* b, int H, int W, int pix, int lo, uint64_t* out, hipStream_t s) {
  const int layout = pix_layout(pix);   // (the colour flags do not enter)
  const bool yuv = pix_is_yuv(pix);
  if (!a || !b || !out || H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 31) || ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3))
    return hipErrorInvalidValue;
  if (lo < 0 || lo > 65535 || (reinterpret_cast<uintptr_t>(out) & 7)) return hipErrorInvalidValue;
  if (layout != FILM_PIX_F32 && layout != FILM_PIX_U8 && !yuv) return hipErrorInvalidValue;
  const PixLayout row = pix_row(pix);
  if (yuv && ((W & row.sx) | (H & row.sy))) return hipErrorInvalidValue;
  DiffParams p{};
  p.a = a; p.b = b; p.lo = (uint32_t)lo; p.out = reinterpret_cast<unsigned long long*>(out);
  auto group = [](int64_t off, int hp, int wp) {
    const int bw = (wp + 7) / 8;
    return DiffGroup{off, hp, wp, bw, (int64_t)((hp + 7) / 8) * bw};
  };
  p.g[0] = group(0, H, W);
  if (yuv) {
    const int hc = H >> row.sy, wc = W >> row.sx;
    p.g[1] = group((int64_t)H * W, hc, wc);                                           // Cb, or the CbCr pairs
    if (!row.semi_planar) p.g[2] = group((int64_t)H * W + (int64_t)hc * wc, hc, wc);   // Cr
  }
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess) e = hipMemsetAsync(out, 0, 12 * sizeof(uint64_t), s);
  if (e != hipSuccess) return e;
  const int64_t units = std::max(p.g[0].units, std::max(p.g[1].units, p.g[2].units));   // (every group's loop starts at lane 0)
  const int64_t grid = std::min<int64_t>((int64_t)std::max(cus, 1) * FILM_DIFF_WG_PER_CU, (units + FILM_DIFF_THREADS - 1) / FILM_DIFF_THREADS);
  auto kernel = layout == FILM_PIX_F32 ? frame_diff_kernel<FILM_PIX_F32> : layout == FILM_PIX_U8 ? frame_diff_kernel<FILM_PIX_U8>
              : layout == FILM_PIX_NV12 ? frame_diff_kernel<FILM_PIX_NV12> : layout == FILM_PIX_P010 ? frame_diff_kernel<FILM_PIX_P010>
              : pix_is_yuv10(pix) ? frame_diff_kernel<FILM_PIX_I010> : frame_diff_kernel<FILM_PIX_I420>;   // (planar: every subsampling)
  static_assert(FILM_DIFF_THREADS == 256, "launch_units starts workgroups of 256");
  return launch_units(kernel, grid * FILM_DIFF_THREADS, s, p);   // `grid` workgroups
}

// ---- the segment copy (a grouped stream's restores and saves; film_kernels.h, SegmentTable) ---------------------------------------------
// (Like the two launchers above, this one stands beside its kernel; launch_units: "host" below.)
namespace {
// lane = one aligned 16-byte vector of the destination per step.  The segment of unit u is the one with unit0[k] <= u < unit0[k + 1]; a
// lane's units grow from step to step, so it walks k forwards from where it stood (empty segments, which own no unit, are passed on the
// way).  The words are moved as uint32: no float is ever interpreted.
__global__ __launch_bounds__(FILM_SEG_THREADS) void segment_copy_kernel(SegmentTable t, const uint32_t* src, uint32_t* dst) {
  const int64_t total = t.unit0[t.n];
  const int64_t step = (int64_t)gridDim.x * FILM_SEG_THREADS;
  int k = 0;
  for (int64_t u = (int64_t)blockIdx.x * FILM_SEG_THREADS + threadIdx.x; u < total; u += step) {
    while (u >= t.unit0[k + 1]) ++k;   // (u < total = unit0[n]: k stays below n)
    const SegmentCopy g = t.seg[k];
    const uint32_t* sp = src + g.src;
    uint32_t* dp = dst + g.dst;
    const int lead = (int)((reinterpret_cast<uintptr_t>(dp) >> 2) & 3);   // floats of the segment's first vector in front of it
    const int64_t j = (u - t.unit0[k]) * 4 - lead;                         // the vector's first float, relative to the segment
    if (j >= 0 && j + 4 <= g.count) {
      uint4 v;
      if ((reinterpret_cast<uintptr_t>(sp + j) & 15) == 0) v = *reinterpret_cast<const uint4*>(sp + j);
      else v = make_uint4(sp[j], sp[j + 1], sp[j + 2], sp[j + 3]);
      *reinterpret_cast<uint4*>(dp + j) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (j + e >= 0 && j + e < g.count) dp[j + e] = sp[j + e];
    }
  }
}
}  // namespace

hipError_t film_launch_segment_copy(const SegmentCopy* segs, int n, const float* src, float* dst, hipStream_t s) {
  if (n < 0 || n > FILM_SEG_MAX || (n > 0 && (!segs || !src || !dst))) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) return hipErrorInvalidValue;
  SegmentTable t{};
  t.n = n;
  for (int k = 0; k < n; ++k) {
    const SegmentCopy& g = segs[k];
    if (g.src < 0 || g.dst < 0 || g.count < 0) return hipErrorInvalidValue;
    t.seg[k] = g;
    const int64_t lead = (int64_t)((reinterpret_cast<uintptr_t>(dst + g.dst) >> 2) & 3);
    t.unit0[k + 1] = t.unit0[k] + (g.count ? (lead + g.count + 3) / 4 : 0);
  }
  const int64_t total = t.unit0[n];
  if (total == 0) return hipSuccess;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  const int64_t grid = std::min<int64_t>((int64_t)std::max(cus, 1) * FILM_SEG_WG_PER_CU, (total + FILM_SEG_THREADS - 1) / FILM_SEG_THREADS);
  static_assert(FILM_SEG_THREADS == 256, "launch_units starts workgroups of 256");
  return launch_units(segment_copy_kernel, grid * FILM_SEG_THREADS, s, t, reinterpret_cast<const uint32_t*>(src), reinterpret_cast<uint32_t*>(dst));   // `grid` workgroups
}

namespace {

// ---- host ----------------------------------------------------------------------------------------------------------------------
// every other kernel of this file: one thread per unit, 256 per workgroup (frame_histogram_kernel: one workgroup per 256 units)
template <class... P, class... A>
hipError_t launch_units(void (*kernel)(P...), int64_t units, hipStream_t s, const A&... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, args...);
  return hipGetLastError();
}

const U8Table& u8_table() {
  static const U8Table tab = [] {
    U8Table t;
    for (int i = 0; i < 256; ++i) t.v[i] = (float)i / 255.0f;
    return t;
  }();
  return tab;
}

// The tables of one colour setting (include/film_hip.h, "The 4:2:0 arithmetic"): built once per setting, on the host.
// matrix: 0 BT.709, 1 BT.601, 2 BT.2020 non-constant luminance
YuvTables make_yuv_tables(int matrix, bool full) {
  YuvTables t;
  const double Kr = matrix == 1 ? 0.299 : matrix == 2 ? 0.2627 : 0.2126, Kb = matrix == 1 ? 0.114 : matrix == 2 ? 0.0593 : 0.0722, Kg = 1.0 - Kr - Kb;
  for (int i = 0; i < 256; ++i) {
    t.y[i] = full ? (float)i / 255.0f : ((float)i - 16.0f) / 219.0f;
    t.c[i] = ((float)i - 128.0f) / (full ? 255.0f : 224.0f);
  }
  YuvMatrix& m = t.m;
  m.a_r = (float)(2.0 * (1.0 - Kr)); m.a_b = (float)(2.0 * (1.0 - Kb));
  m.g_b = (float)(2.0 * Kb * (1.0 - Kb) / Kg); m.g_r = (float)(2.0 * Kr * (1.0 - Kr) / Kg);
  m.kr = (float)Kr; m.kg = (float)Kg; m.kb = (float)Kb;
  m.s_b = (float)(0.5 / (1.0 - Kb)); m.s_r = (float)(0.5 / (1.0 - Kr));
  m.y_scale = full ? 255.0f : 219.0f; m.y_off = full ? 0.0f : 16.0f; m.c_scale = full ? 255.0f : 224.0f;
  return t;
}
// the tables of a public pix value (its FILM_YUV_* flags)
const YuvTables& yuv_tables(int pix) {
  static const YuvTables all[6] = {make_yuv_tables(0, false), make_yuv_tables(0, true), make_yuv_tables(1, false),
                                   make_yuv_tables(1, true),  make_yuv_tables(2, false), make_yuv_tables(2, true)};
  return all[((pix & FILM_YUV_BT601) ? 2 : (pix & FILM_YUV_BT2020) ? 4 : 0) + ((pix & FILM_YUV_FULL) ? 1 : 0)];
}
// The same for a 10-bit layout (include/film_hip.h, "The 10-bit 4:2:0 arithmetic"): the matrix is that of the 8-bit tables, the scales are 10-bit.
Yuv10Consts yuv10_consts(int pix) {
  const bool full = (pix & FILM_YUV_FULL) != 0;
  Yuv10Consts k;
  k.y_sub = full ? 0.0f : 64.0f; k.y_div = full ? 1023.0f : 876.0f; k.c_div = full ? 1023.0f : 896.0f;
  k.m = yuv_tables(pix).m;
  k.m.y_scale = full ? 1023.0f : 876.0f; k.m.y_off = full ? 0.0f : 64.0f; k.m.c_scale = full ? 1023.0f : 896.0f;
  return k;
}

// f(YuvLayout<LAYOUT>()) for the Y'CbCr layout of a pix value: how both launchers below choose their kernel instance (constexpr for the
// static_asserts behind it, which walk its cases at compile time)
template <class F> constexpr hipError_t with_yuv_layout(int pix, F f) {
  switch (pix_layout(pix)) {
    case FILM_PIX_I420: return f(YuvLayout<FILM_PIX_I420>());
    case FILM_PIX_NV12: return f(YuvLayout<FILM_PIX_NV12>());
    case FILM_PIX_I010: return f(YuvLayout<FILM_PIX_I010>());
    case FILM_PIX_P010: return f(YuvLayout<FILM_PIX_P010>());
    case FILM_PIX_I422: return f(YuvLayout<FILM_PIX_I422>());
    case FILM_PIX_I444: return f(YuvLayout<FILM_PIX_I444>());
    case FILM_PIX_I210: return f(YuvLayout<FILM_PIX_I210>());
    case FILM_PIX_I410: return f(YuvLayout<FILM_PIX_I410>());
    default: return hipErrorInvalidValue;
  }
}
// kPixLayouts (film_kernels.h) says what the cases above and the YuvLayout of each say: checked here, over all 256 layout codes
template <class F> constexpr bool every_layout_code(F ok) {
  for (int code = 0; code < 256; code++)
    if (!ok(code, pix_row(code))) return false;
  return true;
}
static_assert(every_layout_code([](int code, PixLayout r) { return (with_yuv_layout(code, [](auto) { return hipSuccess; }) == hipSuccess) == (r.depth != 0); }),
              "with_yuv_layout's cases are the Y'CbCr rows of kPixLayouts");
static_assert(every_layout_code([](int code, PixLayout r) {
                return with_yuv_layout(code, [r](auto l) {
                  using L = decltype(l);
                  return L::PIX == r.code && L::WIDE == (r.depth == 10) && L::SEMI_PLANAR == r.semi_planar && L::SX == r.sx && L::SY == r.sy &&
                         (int)sizeof(typename L::Sample) == r.sample_bytes ? hipSuccess : hipErrorUnknown;
                }) != hipErrorUnknown; }),
              "every YuvLayout's WIDE, SEMI_PLANAR, SX, SY and Sample are its row of kPixLayouts");

}  // namespace

// The one place that launches a cut kernel: float32 frames, or bytes that the cut itself converts (whole aligned 32-bit words: the
// 8-bit kernels read such words).
hipError_t film_launch_cut_tiles(const TileMapParams& p, int pix, hipStream_t s) {
  const bool ov = (p.ovy | p.ovx) != 0;
  if (pix_layout(pix) == FILM_PIX_F32) return launch_units(ov ? frame_to_tiles_kernel<true> : frame_to_tiles_kernel<false>, (int64_t)p.ntiles * p.TH * p.TW * 3, s, p);
  if (p.ntiles <= 0) return hipSuccess;
  if (!pix_is_yuv(pix))
    return launch_units(ov ? frame_u8_to_tiles_kernel<true> : frame_u8_to_tiles_kernel<false>, (int64_t)p.ntiles * p.TH * ((p.TW * 3 + 11) / 12), s, p, u8_table());
  return with_yuv_layout(pix, [&](auto l) {
    using L = decltype(l);
    if ((p.W & L::SX) | (p.H & L::SY)) return hipErrorInvalidValue;   // (a subsampled axis is even)
    return launch_units(ov ? frame_yuv_to_tiles_kernel<true, L::PIX> : frame_yuv_to_tiles_kernel<false, L::PIX>, (int64_t)p.ntiles * p.TH * ((p.TW + 3) / 4), s, p,
                        L::consts(pix));
  });
}

hipError_t film_launch_join_tiles(const TileMapParams& p, hipStream_t s) {
  if (!(p.ovy | p.ovx)) return launch_units(tiles_to_frame_kernel, (int64_t)p.ntiles * p.ph * p.pw * 3, s, p);
  if (p.ntiles <= 0) return hipSuccess;
  // the frames the tile range touches; within one frame only the rows of its block rows
  const int T = p.bh * p.bw, last = p.tile0 + p.ntiles - 1;
  const int b0 = p.tile0 / T, nfr = last / T - b0 + 1;
  int y0 = 0, y1 = p.H;
  if (nfr == 1) {
    y0 = film_tile_origin((p.tile0 % T) / p.bw, p.ph, p.ovy, p.H, p.eh);
    y1 = film_tile_origin((last % T) / p.bw, p.ph, p.ovy, p.H, p.eh) + p.eh;
  }
  return launch_units(blend_tiles_kernel, (int64_t)nfr * (y1 - y0) * p.W * 3, s, p, b0, nfr, y0, y1 - y0);
}

hipError_t film_launch_to_uint8(const float* src, uint8_t* dst, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  return launch_units(to_uint8_kernel, (n + 3) / 4, s, src, dst, n);
}

hipError_t film_launch_rgb_to_yuv(const float* src, void* dst, int H, int W, int pix, hipStream_t s) {
  if (H <= 0 || W <= 0) return hipErrorInvalidValue;
  if (pix_is_yuv10(pix) && (reinterpret_cast<uintptr_t>(dst) & 1)) return hipErrorInvalidValue;
  return with_yuv_layout(pix, [&](auto l) {
    using L = decltype(l);
    if ((W & L::SX) | (H & L::SY)) return hipErrorInvalidValue;   // (a subsampled axis is even)
    return launch_units(rgb_to_yuv_kernel<L::PIX>, (int64_t)((H + 1) / 2) * ((W + 7) / 8), s, src, static_cast<typename L::Sample*>(dst), H, W, L::consts(pix));
  });
}
