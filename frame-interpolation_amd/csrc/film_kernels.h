// film_kernels.h -- parameter blocks and launchers of the gfx950 kernels behind libfilm_hip.so.
//
// Every activation is a pixel-major ("NHWC") float32 buffer [N][H][W][stride]; a kernel reads
// or writes a *channel slice* of such a buffer (pointer pre-offset by the first channel,
// `stride` = floats per pixel of the underlying buffer).  That is how every tf.concat of the
// reference (feature_extractor.py:191, pyramid_flow_estimator.py:95, interpolator.py:167-183,
// fusion.py:136) disappears: producers write straight into their slice of the consumer's input.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/film_hip.h"   // FILM_PIX_*, FILM_YUV_*: the `pix` of the frame I/O launchers

#define FILM_MAX_SEG 4
#define FILM_BK 16  // channels per K-step of the implicit GEMM; every concat segment is a multiple

// One K-segment of a (virtually concatenated) convolution input.
struct ConvSeg {
  const float* ptr;  // [NBs][Hs][Ws][stride], first channel of the segment
  int stride;        // floats per pixel
  int C;             // channels in the segment, multiple of FILM_BK
  int boff, bmod;    // batch remap: b' = b + boff; if (b' >= bmod) b' -= bmod   (bmod = 0: none)
  int up;            // 1: source is (H/2, W/2); nearest-neighbour x2 on read (fusion.py:133-134)
};

// Conv2D(padding='same', stride 1) [+ bias] [+ leaky_relu(0.2)] as implicit GEMM:
//   M = NB*H*W output pixels, N = Cout, K = ksize^2 * Ctot, K ordered (tap, segment, channel).
// Every segment is addressed with 32-bit byte offsets from seg.ptr: the buffer behind it must be < 4 GiB - except in
// conv_wino43_kernel, whose buffer resource starts at the workgroup's own first halo row (any size).
struct ConvParams {
  ConvSeg seg[FILM_MAX_SEG];
  int nseg;
  int ksize;          // 1, 2, 3; TF 'same': pad_before = (ksize-1)/2, rest after
  const float* w;     // the copy of the layer's weights that the kernel family reads (ConvFamilyRow::weights; layouts: kLayouts, film_layers.cpp)
  const float* bias;  // [Cout]
  float* out;         // [NB][H][W][ostride], first output channel
  int ostride;
  int NB, H, W;
  int Cout, Ctot;
  int leaky;
  int M;
  // Sub-pixel fold of nearest-x2-upsample + 2x2 conv (fusion.py:133-135), conv_buf_kernel only.  fold = 1: the
  // launch computes output phase (py, px), i.e. out[2y+py][2x+px] for every pixel (y, x) of the LOW-resolution input
  // (H, W, M describe that grid; the output is 2H x 2W), from `ftaps` taps (tdy[t], tdx[t]) in {0,1}^2 of it, with
  // weights [Cout][ftaps * Ctot] pre-summed over the kernel taps that read the same input pixel.
  // fold = 2: all four phases in ONE launch, phase = blockIdx.z = py*2 + px, taps (a, b) with a <= py, b <= px in
  // raster order, weights of phase q at w + fold_woff[q] (py, px, ftaps, tdy, tdx are then ignored).
  // fold = 3 (conv_fold4_kernel, conv_fold4_impl.h): the same op in its difference form - four GEMMs over K = Ctot on the planes
  // I, Dx, Dy, Dxy of the low-resolution input, combined in the epilogue; weights [Cout/32][chunk of 8][plane 4][K half][32][4]
  // (S, Sx, Sy, W11); py, px, ftaps, tdy, tdx, fold_woff are ignored.
  int fold, py, px, ftaps;
  signed char tdy[4], tdx[4];
  long long fold_woff[4];
  // Split-K (conv_buf_kernel, fold == 0): ksplit > 1 -> blockIdx.z = split s sums the K steps
  // [s * nsteps / ksplit, (s + 1) * nsteps / ksplit) and writes the raw partial sums to part[s][M][Cout]; film_launch_conv
  // then adds the partials in split order, the bias and the activation (conv_splitk_reduce_kernel).  No atomics: the
  // result is a fixed function of (shape, ksplit).  For the deep, small-M layers of the coarse pyramid levels, whose
  // K loop (up to 1080 steps) otherwise runs on a handful of workgroups.
  int ksplit;
  float* part;
  // Unused: it was the tile count of conv_wino2d_kernel's chained-tile variant, whose code is gone.  The field keeps its place, and that kernel's
  // argument batch still loads it, because taking it out moves mg_* / tl_* and renumbers the kernel's scalar registers: to go with a measured A/B.
  int unused_chain;
  // conv_wino2d_kernel, filled by ITS LAUNCHER (callers leave them 0): ceil(2^32 / d) for d = tiles per image, tiles per row, channel blocks of
  // the grid - the workgroup -> (image, tile row, tile column, channel block) decomposition then costs three s_mul_hi_u32 instead of three
  // 40-instruction integer divisions in front of the first DMA request (0: divide; conv_wino2d_impl.h, "prologue diet")
  unsigned mg_tpi, mg_ntx, mg_nby;
  int tl_ntx, tl_tpi;   // ... and the tiles per row / per image themselves
  // Fused AveragePooling2D(2, 2) of the output (feature_extractor.py:138-146: every sub-extractor stage but the last
  // is followed by a pool), conv_wino43_kernel's 64-pixel tiles only: the epilogue also writes
  // pool_out[img][y/2][x/2][n] = (((o(y,x) + o(y,x+1)) + o(y+1,x)) + o(y+1,x+1)) * 0.25 (pool_vec_kernel's order) from
  // the activated outputs it holds in registers - the former pool launch and its re-read of the feature map.  H, W even.
  float* pool_out;    // nullptr: none
  int pool_ostride;
  // Fused 1x1 convolution behind this layer (conv_wino43_kernel, the NH = 1 tiles with BN = Cout = 64: a workgroup holds every
  // channel of its 256 pixels): pw_out[pixel][j] = sum_c act(out[pixel][c]) * pw_w[c][j] + pw_bias[j], one fma chain per output
  // in channel order like conv_pw_kernel; `out` itself is NOT written.  The RGB head of the fusion decoder (fusion.py:138-140).
  const float* pw_w;      // [Cout][pw_cout]; nullptr: none
  const float* pw_bias;
  float* pw_out;
  int pw_ostride, pw_cout;   // pw_cout <= 4
};

// Flow head of a predictor with 32 filters (pyramid_flow_estimator.py:77-83): 1x1 conv Cin -> 16 + leaky_relu,
// then 1x1 conv 16 -> 2, fused: the 16-channel intermediate stays in registers.
struct FlowHeadParams {
  const float* in;
  int istride;
  int Cin;            // multiple of 4
  const float* w3;    // [Cin][16]
  const float* b3;
  const float* w4;    // [16][2]
  const float* b4;
  float* out;         // [M][2]
  int M;
  const float* add;   // optional [M][2]: the upsampled flow of the coarser level; then sum = out + add is stored too
  float* sum;         //          [M][2]  (v = residual + v, pyramid_flow_estimator.py:161 - the former flow_add launch)
};

// 1x1 convolution with a tiny output width (Cout <= 16): flow heads and the RGB head.
struct ConvPwParams {
  const float* in;
  int istride;
  int Cin;            // multiple of 4
  const float* w;     // [Cin][Cout]
  const float* bias;
  float* out;
  int ostride;
  int Cout;
  int leaky;
  int M;              // pixels
  const float* add;   // Cout == 2 only, optional [M][2]: sum = out + add is stored as well (see FlowHeadParams)
  float* sum;
};

// AveragePooling2D(2, 2, 'valid') on a channel slice (util.py:39-40, feature_extractor.py:138-139).
struct PoolParams {
  const float* in;
  int istride;
  float* out;
  int ostride;
  int C;
  int NB, H, W;       // INPUT spatial dims (even)
};

// tf.image.resize(2*v, 2x) bilinear, half-pixel centres (pyramid_flow_estimator.py:155).
struct FlowUpParams {
  const float* in;    // [NB][h][w][2]
  float* out;         // [NB][2h][2w][2]
  int NB, h, w;
};

// v = r + up  (pyramid_flow_estimator.py:161, util.py:114)
struct FlowAddParams {
  const float* a;
  const float* b;
  float* out;
  int64_t n;          // floats
};

// util.warp (util.py:48-82 -> tfa.image.dense_image_warp): backward bilinear gather with
// edge clamp.  flow is (dx,dy); the sampled position is (y + s*flow_y, x + s*flow_x).
struct WarpParams {
  const float* src;
  int sstride;
  int C;              // multiple of 4, or exactly 3
  const float* flow;  // [NB][H][W][2]
  float fscale;       // 1 in the flow estimator, 0.5 for the mid-frame warps (interpolator.py:163-165)
  float* dst;
  int dstride;
  int NB, H, W;
  // Fused tf.image.resize(2*v) of the flow estimator (pyramid_flow_estimator.py:155): when `coarse` is set the flow of
  // this level is bilinear-x2(2 * coarse) ([NB][H/2][W/2][2], same arithmetic as flow_up_kernel) instead of `flow`,
  // and it is written to flow_out [NB][H][W][2] (C % 4 == 0 launches only) - the former flow_up launch.
  const float* coarse;
  float* flow_out;
  // Fused sixteen miscellaneous channels of an aligned-pyramid level (interpolator.py:167-183 warps [image | features] as one
  // tensor and appends the two half flows): dst3[pix] = {warp(src3, 0.5 pack_b) 3, warp(src3b, 0.5 pack_f) 3, 0.5 pack_b 2,
  // 0.5 pack_f 2, 0 x 6}, pixel stride d3stride (multiple of 4, dst3 16-byte aligned), by one thread per pixel in workgroups behind the
  // feature workgroups of a row band - the former
  // warp_c3 x 2 + pack_flow launches.  src3 / src3b: the two images [NB][H][W][3] (pixel stride s3stride), pack_b / pack_f:
  // backward / forward flow [NB][H][W][2].  dst3 == nullptr: none.
  const float* src3;
  const float* src3b;
  int s3stride;
  float* dst3;
  int d3stride;
  const float* pack_b;
  const float* pack_f;
  // One launch for both flow directions / both images of a level (batch n = 0 .. NB - 1 of dst and flow_out): the source image of
  // batch n is (n + src_brot) % NB, its flow (n + flow_brot) % NB (`flow`, not `coarse`); the miscellaneous channels exist for the
  // first misc_nb batches only (0: for all NB).
  int src_brot = 0, flow_brot = 0, misc_nb = 0;
};

// Writes channels [6..15] of the 16-wide "misc" group of an aligned-pyramid level:
// backward_flow*0.5 (2), forward_flow*0.5 (2), zeros (6)  (interpolator.py:163-165,182-183).
struct PackFlowParams {
  const float* bflow;  // [B][H][W][2]
  const float* fflow;
  float* dst;          // first misc channel + 6
  int dstride;
  int64_t npix;
};

// Interpolator.__call__ data movement (eval/interpolator.py:30-63 _pad_to_align, :66-126 image_to_patches /
// patches_to_image, :192-206): frame [B][H][W][3] <-> tiles [B*bh*bw][TH][TW][3], tile n = (b, ty, tx) row-major,
// each patch (H/bh x W/bw) zero-padded to (TH, TW) with the patch at offset (oy, ox) = (pad_h//2, pad_w//2).
struct TileMapParams {
  const float* src;
  float* dst;
  int B, H, W;       // frame
  int bh, bw;        // blocks per frame
  int ph, pw;        // patch = H/bh x W/bw
  int TH, TW;        // padded tile
  int oy, ox;        // patch offset inside the tile
  int tile0, ntiles; // tiles [tile0, tile0 + ntiles) of the frame batch are in the tile buffer
  // Overlapped tiles (options "block_overlap_h" / "block_overlap_w"; read by the overlapped cuts and the cross-fade only): tile (ty, tx) holds the
  // eh x ew pixels of the frame from (film_tile_origin(ty, ph, ovy, H, eh), film_tile_origin(tx, pw, ovx, W, ew)), at (oy, ox) of
  // the padded tile.  ovy = ovx = 0: eh = ph, ew = pw, the patches above.
  int ovy, ovx;      // resolved overlap per axis
  int eh, ew;        // tile content = ph + 2 ovy x pw + 2 ovx
};
// First frame row (column) of overlapped tile i of an axis of n pixels cut into patches of p: the patch grown by o on both sides, moved
// inwards at the frame's edge so that every tile has e = p + 2 o pixels.
__host__ __device__ inline int film_tile_origin(int i, int p, int o, int n, int e) {
  const int s = i * p - o;
  return s < 0 ? 0 : (s > n - e ? n - e : s);
}

// Tile id = shape index + CONV_TILE_XCD when the XCD-contiguous block mapping is used.
enum ConvTile { TILE_128x128 = 0, TILE_256x64 = 1, TILE_256x32 = 2, TILE_64x64 = 3, TILE_128x32 = 4,
                TILE_128x64 = 5, TILE_256x128 = 6 /* 8 waves, 4x2 */, TILE_SHAPES = 7,
                TILE_C3_DIRECT = 7 /* with CONV_TILE_C3: conv_c3_kernel (no LDS, weights in registers, conv_c3_impl.h) */, CONV_TILE_XCD = 16,
                CONV_TILE_C3 = 32 /* first-layer mode: 3-channel image input, [48][Cout] weights */,
                CONV_TILE_HALO = 64 /* conv_halo_kernel: shape index = HaloTile, weights [Cout][chunk][tap][16] */,
                CONV_TILE_WINO = 256 /* conv_wino_kernel (F(2,3) along x): shape index = WinoTile, weights
                                        [Cout][chunk of 8][nu*3+dy][8] */,
                CONV_TILE_SPLIT = 128 /* conv_halo_split_kernel (precision mode bf16x6): shape index = HaloTile,
                                         weights [Cout][chunk][tap][3 planes][16] bf16 */,
                CONV_TILE_X3 = 512 /* precision mode bf16x3.  With CONV_TILE_SPLIT: conv_halo_split_kernel on planes hi, mid with
                                      three products; with CONV_TILE_WINO: conv_winox3_kernel, shape index = WinoX3Tile,
                                      weights [Cout][chunk][dy][j][h][plane][16] bf16 */,
                CONV_TILE_F43 = 2048 /* with CONV_TILE_WINO: conv_wino43_kernel (F(4,3) along x, fp32): shape index = Wino43Tile,
                                        weights [Cout][chunk of 8][dy][nu 6][8] */,
                CONV_TILE_W2D = 8192 /* conv_wino2d_kernel (nested F(4,3)x x F(2,3)y, fp32): shape index = Wino2dTile, weights
                                        [Cout/32][chunk of 8][mu 4][nu 6][K half][32][4] */,
                CONV_TILE_EXT = 4096 /* conv_wino43_kernel: shape index = (tile & 15) + 16 */,
                CONV_TILE_FOLD4 = 16384 /* conv_fold4_kernel (nearest x2 upsample + 2x2 conv in its difference form, fp32): shape index =
                                           Fold4Tile, weights [Cout/32][chunk of 8][plane 4][K half][32][4] */,
                CONV_TILE_FOLDX3 = 1024 /* conv_foldx3_kernel (precision mode bf16x3, folded upsample + 2x2): shape index =
                                           FoldX3Tile, weights [Cout][chunk][9 (tap, phase) steps][plane][16] bf16 */ };
// conv_wino43_kernel tiles (CONV_TILE_WINO | CONV_TILE_F43): patch rows x 128 pixels x output channels, wave block TM x TN
// 0-2: 128-pixel patches, 8 waves, one workgroup per CU; 3-5 ("Q16"): 64-pixel patches (an MFMA row tile = two patch rows x 16
// quads), 4 waves, 72 / 54 KB of LDS -> two workgroups per CU.  Same k-ordered sums: the autotuner picks freely among them.
enum Wino43Tile { W43_4x64_T21 = 0, W43_4x64_T12 = 1, W43_4x32_T11 = 2, W43_Q16_4x64_T21 = 3, W43_Q16_4x64_T12 = 4, W43_Q16_4x32_T11 = 5,
                  W43_Q16_4x64_N1 = 6 /* a wave owns all six nu planes of one 32x32 tile: no epilogue exchange */,
                  /* the Q16 tiles with the activation loads requested two K chunks ahead (second register set) */
                  W43_Q16_4x64_T21_P2 = 7, W43_Q16_4x64_T12_P2 = 8, W43_Q16_4x32_T11_P2 = 9, W43_Q16_4x64_N1_P2 = 10,
                  /* the 32-channel Q16 tile with the weight fragments read straight from global memory (no weight ring: 36 KB of
                     LDS, <= 128 VGPRs -> FOUR workgroups per CU; the short K loops of the 32-channel layers are latency bound) */
                  W43_Q16_4x32_T11_BG = 11,
                  /* "Q8": 32-pixel patches, 8 rows (an MFMA row tile = FOUR patch rows x 8 quads): the same 256 pixels per
                     workgroup, no empty quads on the 15 * 2^k wide levels, 10 halo rows per 8 output rows; all with the
                     activation loads two chunks ahead */
                  W43_Q8_8x64_T21_P2 = 12, W43_Q8_8x64_N1_P2 = 13, W43_Q8_8x32_T11_BG = 14, W43_Q8_8x64_T12_P2 = 15,
                  /* ids >= 16 carry CONV_TILE_EXT in the tile id (shape = (tile & 15) + 16).  The 32-channel Q8 tile WITH the
                     weight ring: 48 KB of LDS, 152 VGPRs -> three workgroups per CU (flow level 0 conv_0: -7 % against the BG tile) */
                  W43_Q8_8x32_T11_P2 = 16 };
// this build of the library holds the opt-in kernel families (and Wino43Tile shapes): FILM_EXTRA_FAMILIES=1 (Makefile EXTRA=1)
#ifdef FILM_EXTRA_FAMILIES
constexpr bool kExtraFamilies = true;
#else
constexpr bool kExtraFamilies = false;
#endif
// the Wino43Tile shapes this build of the library instantiates (conv_igemm.hip): all of them with FILM_EXTRA_FAMILIES, seven without
static inline bool film_w43_shape_built(int sh) {
  if (kExtraFamilies) return sh >= 0 && sh <= W43_Q8_8x32_T11_P2;
  return sh == W43_Q16_4x64_T21_P2 || sh == W43_Q16_4x32_T11_P2 || sh == W43_Q16_4x64_N1_P2 || sh == W43_Q8_8x64_T21_P2 || sh == W43_Q8_8x64_N1_P2 ||
         sh == W43_Q8_8x32_T11_BG || sh == W43_Q8_8x32_T11_P2;
}
// conv_wino2d_kernel tiles (CONV_TILE_W2D): one 32-unit MFMA tile (unit = 2 rows x 4 pixels; 8 rows x 32 pixels) x output channels;
// 64 channels = 8 waves (one workgroup per CU), 32 channels = 4 waves (two per CU).  Same sums: the autotuner picks freely.
// W2D_8x32_S2 (round 6): the 32-channel tile on TWO DMA stages instead of three (48 KB of LDS; all requests of a super-chunk in the gaps of ONE
// chunk, one super-chunk less requested in the prologue): 4-15 % faster on every layer with K <= 208, equal above (profiles/r06_w2d_chain_ns2.log).
// W2D_16x* (round 6): the 32 units as 8 unit rows x 4 units = 16 x 16 pixels (W2D_F_SQ, conv_wino2d_impl.h).  Offered where it pads a level no more than the 8 x 32
// arrangement: a 144x240 level tiles exactly (8 x 32: 7.5 tiles per row) - 5-7.5 % faster there, and the autotuner also picks it on some exact-fit levels
// (profiles/r06_w2d_square_tile.log).
enum Wino2dTile { W2D_8x64 = 0, W2D_8x32 = 1, W2D_8x32_S2 = 2, W2D_16x64 = 3, W2D_16x32 = 4, W2D_16x32_S2 = 5, W2D_SHAPES = 6 };
inline bool film_w2d_square(int shape) { return shape >= W2D_16x64 && shape <= W2D_16x32_S2; }
inline bool film_w2d_64(int shape) { return shape == W2D_8x64 || shape == W2D_16x64; }
// conv_fold4_kernel tiles (CONV_TILE_FOLD4): 4 rows x 32 low-resolution pixels x output channels; four waves side by side, each 4 x 8 pixels
// x all channels of the tile.  64 channels: 235 VGPRs, two workgroups per CU; 32 channels: 139 VGPRs, three.  Same sums.
enum Fold4Tile { F4_4x64 = 0, F4_4x32 = 1 };
// conv_foldx3_kernel tiles (CONV_TILE_FOLDX3): low-resolution patch rows x 32 pixels x output channels (waves M x N)
enum FoldX3Tile { FX3_4x64 = 0 /* 4x1 */, FX3_8x64 = 1 /* 8x1 */, FX3_4x128 = 2 /* 4x2 */ };
// conv_winox3_kernel tiles (CONV_TILE_WINO | CONV_TILE_X3): patch rows x 64 pixels x output channels, wave block TM x TN
enum WinoX3Tile { WX3_4x128_T22 = 0, WX3_4x64_T12 = 1, WX3_4x64_T21 = 3, WX3_4x32_T11 = 4 };   // all 8 waves
// conv_wino_kernel tiles: patch rows x 64 pixels x output channels (waves M x N)
enum WinoTile { WINO_4x128 = 0 /* 4x2 */, WINO_4x64 = 1 /* 4x1 */, WINO_4x128_W16 = 2 /* 4x4: 16 waves */,
                WINO_4x64_W8 = 3 /* 4x2: 32 channels per wave */, WINO_4x32 = 4 /* 4x1 */, WINO_8x64_W16 = 5 /* 8x2 */,
                WINO_8x32_W8 = 6 /* 8x1 */, WINO_2x64 = 7 /* 2x2 */, WINO_SHAPES = 8 };
// conv_halo_kernel tiles: patch rows x 32 pixels x output channels (waves M x N)
enum HaloTile { HALO_8x128 = 0 /* 4x2 */, HALO_8x64 = 1 /* 4x1 */, HALO_8x32 = 2 /* 4x1 */, HALO_4x64 = 3 /* 4x1 */,
                HALO_4x128 = 4 /* 2x2 */, HALO_4x32 = 5 /* 4x1 */, HALO_SHAPES = 6 };

struct TileShape { int bm, bn; };
static inline TileShape film_tile_shape(int tile) {
  switch (tile & (CONV_TILE_XCD - 1)) {
    case TILE_128x128: return {128, 128};
    case TILE_256x64: return {256, 64};
    case TILE_256x32: return {256, 32};
    case TILE_64x64: return {64, 64};
    case TILE_128x64: return {128, 64};
    case TILE_256x128: return {256, 128};
    default: return {128, 32};
  }
}

// ---- Convolution kernel families --------------------------------------------------------------------------------------------
// Every convolution op runs on one family (kernels: see the CONV_TILE_* flags above); its tile id = the family's flag bits | shape
// index [| CONV_TILE_XCD].  Tile ids are an external format (plan and profile JSON, tune caches): the bits above do not change.
enum ConvFamily { FAM_BUF /* also fold = 2 */, FAM_C3, FAM_W2D, FAM_W43, FAM_FOLD4 /* fold = 3 */,        // the default library
                  FAM_HALO, FAM_SPLIT6, FAM_SPLIT3, FAM_WINO, FAM_WINOX3, FAM_FOLDX3 /* fold = 2 */,       // FILM_EXTRA_FAMILIES only
                  CONV_FAMILIES };
constexpr int CONV_TILE_FAMILY = CONV_TILE_C3 | CONV_TILE_HALO | CONV_TILE_SPLIT | CONV_TILE_WINO | CONV_TILE_X3 | CONV_TILE_FOLDX3 |
                                 CONV_TILE_F43 | CONV_TILE_W2D | CONV_TILE_FOLD4;

// Float offsets into the packed weights of the layouts a convolution kernel reads (kLayouts, film_layers.cpp), -1: the layer has none.
// LayerPack and OpDesc (film_internal.h) both carry them; a family's row names the one its kernel reads.
struct ConvWeights {
  int64_t w_off = 0;      // K-major [Cout][kh*kw*ctot] (first layer: [48][Cout]); an op's conv_buf_kernel weights (fold = 2: the phases)
  int64_t wh_off = -1;    // 3x3 K-major layers: the conv_halo_kernel copy, [Cout][ctot/16][9][16]
  int64_t ws_off = -1;    // ... the bf16x6 copy for conv_halo_split_kernel, [Cout][ctot/16][9][3][16] bf16 (offset in floats; 1.5 floats per weight)
  int64_t ww_off = -1;    // ... the F(2,3)-along-x transformed copy for conv_wino_kernel, [Cout][ctot/8][12][8]
  int64_t wx_off = -1;    // ... and that copy split into bf16 hi / mid for conv_winox3_kernel, [Cout][ctot/16][dy][j][h][plane][16] bf16 (nu = 2h + j)
  int64_t w43_off = -1;   // ... the F(4,3)-along-x transformed copy for conv_wino43_kernel, [Cout][ctot/8][3 dy][6 nu][8]
  int64_t w2d_off = -1;   // LayerPack::has_w2d() layers: the nested F(4,3)x x F(2,3)y copy for conv_wino2d_kernel, [Cout/32][ctot/8][mu 4][nu 6][K half][32][4]
  int64_t wfx_off = -1;   // 2x2 layers behind a nearest upsample: the phase-summed weights as bf16 hi / mid for conv_foldx3_kernel
  int64_t wf4_off = -1;   // ... the four planes S, Sx, Sy, W11 of the difference form for conv_fold4_kernel, [Cout/32][ctot/8][plane 4][K half][32][4]
};

namespace film_internal {   // the autotune candidates of each family (film_tune.cpp)
struct OpDesc;
std::vector<int> tile_candidates(const OpDesc&), c3_candidates(const OpDesc&), wino2d_candidates(const OpDesc&), wino43_candidates(const OpDesc&),
    fold4_candidates(const OpDesc&), halo_candidates(const OpDesc&), wino_candidates(const OpDesc&), winox3_candidates(const OpDesc&),
    foldx3_candidates(const OpDesc&);
}  // namespace film_internal
struct ConvFamilyRow {
  int flags;                            // tile-id bits: tile & CONV_TILE_FAMILY
  int64_t ConvWeights::* weights;       // the weight copy its kernel reads
  bool splitk;                          // implements ConvParams::ksplit
  bool in_default;                      // in the default library (else FILM_EXTRA_FAMILIES only)
  int fused_shape;                      // >= 0: fuses a 2x2 pool / 1x1 head into its epilogue; this shape carries the RGB head (Cout = 64)
  std::vector<int> (*candidates)(const film_internal::OpDesc&);
  int (*default_shape)(int Cout, int64_t M);   // shape before autotuning, M = output pixels of the launch
};

// default shapes: conv_buf_kernel's largest tile that still gives >= 768 workgroups, conv_halo_split_kernel's
constexpr int conv_buf_shape(int Cout, int64_t M) {
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * (Cout / bn); };
  if (Cout % 128 == 0) return blocks(128, 128) >= 768 ? TILE_128x128 : TILE_64x64;
  if (Cout % 64 == 0) return blocks(256, 64) >= 768 ? TILE_256x64 : TILE_64x64;
  return blocks(256, 32) >= 768 ? TILE_256x32 : TILE_128x32;
}
constexpr int film_split_shape(int Cout, int64_t) { return Cout % 128 == 0 ? HALO_8x128 : Cout % 64 == 0 ? HALO_4x64 : HALO_8x32; }

inline constexpr ConvFamilyRow kConvFamily[CONV_FAMILIES] = {
  /* FAM_BUF    */ {0, &ConvWeights::w_off, true, true, -1, film_internal::tile_candidates, conv_buf_shape},
  /* FAM_C3     */ {CONV_TILE_C3, &ConvWeights::w_off, false, true, -1, film_internal::c3_candidates, [](int, int64_t) -> int { return TILE_C3_DIRECT; }},
  /* FAM_W2D    */ {CONV_TILE_W2D, &ConvWeights::w2d_off, true, true, W2D_8x64, film_internal::wino2d_candidates, [](int c, int64_t) -> int { return c % 64 == 0 ? W2D_8x64 : W2D_8x32; }},
  /* FAM_W43    */ {CONV_TILE_WINO | CONV_TILE_F43, &ConvWeights::w43_off, true, true, W43_Q16_4x64_N1_P2, film_internal::wino43_candidates, [](int c, int64_t) -> int { return c % 64 == 0 ? W43_Q16_4x64_T21_P2 : W43_Q16_4x32_T11_P2; }},
  /* FAM_FOLD4  */ {CONV_TILE_FOLD4, &ConvWeights::wf4_off, true, true, -1, film_internal::fold4_candidates, [](int c, int64_t) -> int { return c % 64 == 0 ? F4_4x64 : F4_4x32; }},
  /* FAM_HALO   */ {CONV_TILE_HALO, &ConvWeights::wh_off, false, false, -1, film_internal::halo_candidates, [](int c, int64_t) -> int { return c % 64 == 0 ? HALO_4x64 : HALO_8x32; }},
  /* FAM_SPLIT6 */ {CONV_TILE_SPLIT, &ConvWeights::ws_off, false, false, -1, film_internal::halo_candidates, film_split_shape},
  /* FAM_SPLIT3 */ {CONV_TILE_SPLIT | CONV_TILE_X3, &ConvWeights::ws_off, false, false, -1, film_internal::halo_candidates, film_split_shape},
  /* FAM_WINO   */ {CONV_TILE_WINO, &ConvWeights::ww_off, false, false, -1, film_internal::wino_candidates, [](int c, int64_t) -> int { return c % 64 == 0 ? WINO_4x64_W8 : WINO_4x32; }},
  /* FAM_WINOX3 */ {CONV_TILE_WINO | CONV_TILE_X3, &ConvWeights::wx_off, false, false, -1, film_internal::winox3_candidates, [](int c, int64_t) -> int { return c % 128 == 0 ? WX3_4x128_T22 : c % 64 == 0 ? WX3_4x64_T12 : WX3_4x32_T11; }},
  /* FAM_FOLDX3 */ {CONV_TILE_FOLDX3, &ConvWeights::wfx_off, false, false, -1, film_internal::foldx3_candidates, [](int, int64_t) -> int { return FX3_4x64; }},
};

constexpr bool conv_family_built(int f) { return kConvFamily[f].in_default || kExtraFamilies; }
constexpr int conv_family_of(int tile) {   // -1: no family
  for (int f = 0; f < CONV_FAMILIES; ++f) if ((tile & CONV_TILE_FAMILY) == kConvFamily[f].flags) return f;
  return -1;
}
// tile id of a shape of family f, and back (Wino43Tile shapes >= 16 go into the low four bits with CONV_TILE_EXT: bit 4 is CONV_TILE_XCD)
constexpr int conv_tile(int f, int shape, bool xcd) { return kConvFamily[f].flags | (shape & 15) | (shape >= 16 ? CONV_TILE_EXT : 0) | (xcd ? CONV_TILE_XCD : 0); }
constexpr int conv_tile_shape(int tile) { return (tile & 15) + ((tile & CONV_TILE_EXT) ? 16 : 0); }
// the tile an op of family f starts from (and keeps without autotuning)
constexpr int conv_default_tile(int f, int Cout, int64_t M) { return conv_tile(f, kConvFamily[f].default_shape(Cout, M), true); }

hipError_t film_launch_conv(const ConvParams& p, int tile, hipStream_t s);
hipError_t film_launch_conv_pw(const ConvPwParams& p, hipStream_t s);
hipError_t film_launch_flow_head(const FlowHeadParams& p, hipStream_t s);
hipError_t film_launch_pool(const PoolParams& p, hipStream_t s);
hipError_t film_launch_flow_up(const FlowUpParams& p, hipStream_t s);
hipError_t film_launch_flow_add(const FlowAddParams& p, hipStream_t s);
hipError_t film_launch_warp(const WarpParams& p, hipStream_t s);
hipError_t film_launch_pack_flow(const PackFlowParams& p, hipStream_t s);
// frame_kernels.hip: frame I/O.  `pix` is the public value (include/film_hip.h): a layout in bits 0-7 plus FILM_YUV_BT601 / FILM_YUV_BT2020 /
// FILM_YUV_FULL for the Y'CbCr layouts; the launchers decode it.  Overlapped tiles and their cross-fade when p.ovy | p.ovx.
// What a pix value says, for the launchers, film_engine.cpp and the host-only build alike, is one row of kPixLayouts, in the order of the codes (the
// order a refusal lists them in): depth 0 for the two RGB layouts, else the bits of a Y'CbCr code (10-bit codes lie in 16-bit samples); a chroma plane
// of an H x W frame is [H >> sy][W >> sx] - 4:2:0 (1, 1), 4:2:2 (1, 0), 4:4:4 (0, 0) -, or the two are one plane of CbCr pairs (semi_planar).
struct PixLayout { int code; const char* name; int depth, sample_bytes, sx, sy; bool semi_planar; };
#define FILM_PIX_ROW(NAME, ...) {FILM_PIX_##NAME, "FILM_PIX_" #NAME, __VA_ARGS__}
constexpr PixLayout kPixLayouts[] = {
  FILM_PIX_ROW(F32, 0, (int)sizeof(float), 0, 0, false), FILM_PIX_ROW(U8, 0, 1, 0, 0, false),
  FILM_PIX_ROW(I420, 8, 1, 1, 1, false),  FILM_PIX_ROW(NV12, 8, 1, 1, 1, true),   FILM_PIX_ROW(I422, 8, 1, 1, 0, false),  FILM_PIX_ROW(I444, 8, 1, 0, 0, false),
  FILM_PIX_ROW(I010, 10, 2, 1, 1, false), FILM_PIX_ROW(P010, 10, 2, 1, 1, true),  FILM_PIX_ROW(I210, 10, 2, 1, 0, false), FILM_PIX_ROW(I410, 10, 2, 0, 0, false),
};
#undef FILM_PIX_ROW
constexpr int pix_layout(int pix) { return pix & 0xff; }
constexpr PixLayout pix_row(int pix) {
  for (const PixLayout& r : kPixLayouts)
    if (r.code == pix_layout(pix)) return r;
  return {-1, "", 0, (int)sizeof(float), 0, 0, false};   // what check_pix refuses: no Y'CbCr layout, float32 samples, no chroma shifts
}
constexpr bool pix_is_yuv(int pix) { return pix_row(pix).depth != 0; }
constexpr bool pix_is_yuv10(int pix) { return pix_row(pix).depth == 10; }   // 16-bit samples
constexpr int pix_sample_bytes(int pix) { return pix_row(pix).sample_bytes; }
struct ChromaShift { int sx, sy; };
constexpr ChromaShift pix_chroma_shift(int pix) { return {pix_row(pix).sx, pix_row(pix).sy}; }
// "FILM_PIX_I420 (16), FILM_PIX_NV12 (17), ... or FILM_PIX_I410 (40)": the layouts as a refusal names them, all ten or the Y'CbCr ones
inline std::string pix_layout_list(bool yuv_only) {
  std::string s;
  for (const PixLayout& r : kPixLayouts)
    if (r.depth || !yuv_only)
      s += (s.empty() ? "" : &r == std::end(kPixLayouts) - 1 ? " or " : ", ") + std::string(r.name) + " (" + std::to_string(r.code) + ")";
  return s;
}
// pad + image_to_patches of tiles [tile0, tile0 + ntiles): p.src is float32 [B][H][W][3] (FILM_PIX_F32), or bytes that the cut converts - [B][H][W][3]
// (FILM_PIX_U8: float32(byte) / 255.0f, correctly rounded) or 4:2:0 frames of H * W * 3 / 2 bytes each (FILM_PIX_I420 / NV12; H and W even),
// or 10-bit 4:2:0 frames of H * W * 3 / 2 little-endian uint16 samples each (FILM_PIX_I010 / P010; H and W even, the pointer 4-byte aligned),
// or planar 4:2:2 / 4:4:4 frames of 2 H W / 3 H W samples each (FILM_PIX_I422 / I444: bytes; I210 / I410: uint16; 4:2:2: W even; frame b at sample
// b * S, the batch pointer 4-byte aligned).
hipError_t film_launch_cut_tiles(const TileMapParams& p, int pix, hipStream_t s);
// crop + patches_to_image, or crop + cross-fade.  The cross-fade adds to what the tiles below tile0 left in dst, so the launches of one
// frame go in tile order on one stream.
hipError_t film_launch_join_tiles(const TileMapParams& p, hipStream_t s);
// write_image's rounding on the device: dst[i] = uint8(clip(src[i] * 255, 0, 255) + 0.5)  (eval/util.py:51-52)
hipError_t film_launch_to_uint8(const float* src, uint8_t* dst, int64_t n, hipStream_t s);
// float32 [H][W][3] -> one Y'CbCr frame (clip, matrix, the chroma mean of the subsampling - 2 x 2, 1 x 2 or none -, quantisation): bytes for
// the 8-bit layouts, uint16 for the 10-bit ones (dst then 2-byte aligned, else hipErrorInvalidValue).
hipError_t film_launch_rgb_to_yuv(const float* src, void* dst, int H, int W, int pix, hipStream_t s);
// The sample histogram of one frame (include/film_hip.h, "Scene cuts"): hist[p * 256 + v] = the samples of plane p with 8-bit code v.  The launcher
// zeroes the 768 counters first: a call overwrites.  `frame` is 4-byte aligned and its allocation a whole number of 32-bit words (as for the 8-bit
// cuts).  A lane reads FILM_HIST_VEC_BYTES per step; the grid is min(what the frame needs, FILM_HIST_WG_PER_CU workgroups per compute unit) of
// FILM_HIST_THREADS lanes with a grid-stride loop, so one pass of the full grid covers CUs * WG_PER_CU * THREADS * VEC_BYTES bytes.
#define FILM_HIST_BINS 768
#define FILM_HIST_THREADS 256
#define FILM_HIST_WG_PER_CU 2
#define FILM_HIST_VEC_BYTES 16
hipError_t film_launch_frame_histogram(const void* frame, int H, int W, int pix, uint32_t* hist, hipStream_t s);
// The 8 x 8 block SADs of two frames of one pixel type (include/film_hip.h, "Duplicate frames"): out[p] = {total, max, over, blocks} of plane p,
// `over` counting the blocks whose SAD is > lo (0 .. 65535, stored-code units).  The launcher zeroes the 96 bytes first: a call overwrites.  `a`
// and `b` are 4-byte aligned, `out` 8-byte aligned; refusals as film_launch_frame_histogram.  A lane takes one block position (the blocks of
// the planes that interleave there) per step; the grid is min(what the frame needs, FILM_DIFF_WG_PER_CU workgroups per compute unit) of
// FILM_DIFF_THREADS lanes with grid-stride loops, so one pass of the full grid covers CUs * WG_PER_CU * THREADS block positions per plane group.
// (One workgroup per compute unit: every workgroup ends in up to twelve atomics on one 96-byte line, and at 4K - 507 to 761 workgroups when uncapped -
// two random frames measured 31 - 35 us with a cap of 4 or 2 and 20 - 24 us with 1; 1080p needs fewer than 256 workgroups and does not change.
// profiles/dedup_bench.log, last block.)
#define FILM_DIFF_THREADS 256
#define FILM_DIFF_WG_PER_CU 1
hipError_t film_launch_frame_diff(const void* a, const void* b, int H, int W, int pix, int lo, uint64_t* out, hipStream_t s);
// One launch copies up to FILM_SEG_MAX segments of floats, segment k: dst[seg[k].dst .. + count) = src[seg[k].src .. + count), bit for bit (a
// grouped stream's restores and saves: film_stream.cpp).  The table travels in the kernel arguments.  Units are the ALIGNED 16-byte vectors of
// the destination that hold at least one float of a segment, numbered through all segments (unit0: the prefix sums) and walked by one
// grid-stride loop with 64-bit indices: a vector wholly inside its segment is one 16-byte store - fed by one 16-byte load where the source
// is aligned with it, else by four scalar loads -, the first and the last vector of a segment that starts or ends inside one are copied
// float by float.  Segments may start at any float offset and have any length (0: nothing is copied); they must not overlap each other.
// The grid is min(what the table needs, FILM_SEG_WG_PER_CU workgroups per compute unit) of FILM_SEG_THREADS lanes.
#define FILM_SEG_MAX 32
#define FILM_SEG_THREADS 256
#define FILM_SEG_WG_PER_CU 8
struct SegmentCopy { int64_t src, dst, count; };   // float offsets from the two base pointers, floats
struct SegmentTable {
  SegmentCopy seg[FILM_SEG_MAX];
  int64_t unit0[FILM_SEG_MAX + 1];   // unit0[k] .. unit0[k + 1]: the units of segment k (filled by the launcher)
  int n;
};
// n segments (0 .. FILM_SEG_MAX; more: hipErrorInvalidValue, as are a negative offset or count and a pointer that is not 4-byte aligned)
hipError_t film_launch_segment_copy(const SegmentCopy* segs, int n, const float* src, float* dst, hipStream_t s);
// fills n floats with a deterministic pseudo-random pattern in [-1, 1) (autotune inputs only)
hipError_t film_launch_fill_random(float* dst, int64_t n, uint32_t seed, hipStream_t s);

// metrics_kernels.hip: the per-image metrics of film_image_metrics (eval/metrics.py) on float32 NHWC [B][H][W][C] images, C = 1 or 3
#define FILM_SSIM_TAPS 11
struct MetricsParams {
  const float* pred;    // [B][H][W][C]; clipped to [0,1] on read with FILM_METRIC_CLIP
  const float* ref;     // [B][H][W][C]
  int B, H, W, C;
  int flags;            // FILM_METRIC_* (include/film_hip.h)
  double g[FILM_SSIM_TAPS];   // normalised Gaussian window (metrics._gauss_window), computed on the host
  double c1, c2;        // (k1 max_val)^2, (k2 max_val)^2
  // layout (film_metrics_layout): per image, sum_blocks x 3 partial sums, then C x ssim_tiles_y x ssim_tiles_x ssim partials
  int sum_blocks, ssim_tiles_x, ssim_tiles_y;
  int64_t part_per_image;
  double* part;         // B * part_per_image doubles of scratch
  double* out;          // [B][4]: sum |d|, sum d*d (float32 d), sum of squared float64 differences, ssim
};
void film_metrics_layout(MetricsParams& p);   // fills sum_blocks, ssim_tiles_x / _y and part_per_image from H, W, C
hipError_t film_launch_image_metrics(const MetricsParams& p, hipStream_t s);
