// film_layers.cpp -- the layer table of film_net (names, HWIO shapes, channel permutations of the concatenated inputs) and the
// packer that turns the HWIO tensors into the kernels' weight layouts (K-major, F(4,3), nested F(4,3) x F(2,3), phase-summed
// 2x2, F(2,3), halo, bf16 splits), in contiguous groups that are packed and uploaded on demand; the C-ABI entry points that
// take / give weights (film_set_weight, film_finalize, film_export_packed / film_import_packed, film_export_layouts) and the
// crc32c helper of the SavedModel reader.  Replaces the variable-restore half of tf.saved_model.load (eval/interpolator.py:148).
#include "film_internal.h"

#include <dlfcn.h>

namespace film_internal {

// ---------------------------------------------------------------------------------------------
// Architecture helpers (mirror frame-interpolation_amd/film_hip/weights.py)
// ---------------------------------------------------------------------------------------------
std::vector<int> feature_channels(const film_config& c) {  // feature_extractor.py:186-193
  std::vector<int> out;
  for (int l = 0; l < c.pyramid_levels; ++l) {
    int ch = 0;
    for (int j = 0; j < c.sub_levels; ++j)
      if (j <= l) ch += c.filters << j;
    out.push_back(ch);
  }
  return out;
}
int slot_offset(const film_config& c, int j) {  // channel offset of sub-pyramid stage j in a feature level
  int o = 0;
  for (int k = 0; k < j; ++k) o += c.filters << k;
  return o;
}
std::vector<int> fusion_filters(const film_config& c) {  // fusion.py:75-79
  std::vector<int> out;
  for (int i = 0; i < c.fusion_pyramid_levels - 1; ++i)
    out.push_back(i < c.specialized_levels ? (c.filters << i) : (c.filters << c.specialized_levels));
  return out;
}
std::string predictor_prefix(const film_config& c, int level) {  // pyramid_flow_estimator.py:109-123
  if (level < c.specialized_levels) return "predict_flow/flow_predictor_" + std::to_string(level);
  return "predict_flow/flow_predictor_shared";
}
int predictor_index(const film_config& c, int level) { return std::min(level, c.specialized_levels); }

int validate_config(film_t* h, const film_config& c) {
  if (c.pyramid_levels < 1 || c.pyramid_levels > 12) return fail(h, FILM_ERR_INVALID, "pyramid_levels out of range");
  if (c.pyramid_levels < c.fusion_pyramid_levels || c.fusion_pyramid_levels < 2)
    return fail(h, FILM_ERR_INVALID, "config.pyramid_levels must be greater than or equal to config.fusion_pyramid_levels.");
  if (c.specialized_levels < 1 || c.specialized_levels > c.pyramid_levels || c.specialized_levels > FILM_MAX_SPECIALIZED)
    return fail(h, FILM_ERR_INVALID, "specialized_levels out of range");
  if (c.sub_levels < 1 || c.sub_levels > c.specialized_levels + 1)
    return fail(h, FILM_ERR_INVALID, "sub_levels must be within [1, specialized_levels+1]");
  if (c.filters <= 0 || c.filters % 32) return fail(h, FILM_ERR_INVALID, "filters must be a positive multiple of 32");
  for (int i = 0; i <= c.specialized_levels; ++i) {
    int nf = c.flow_filters[i];
    if (nf <= 0 || nf % 32 || !(nf / 2 == 16 || (nf / 2) % 32 == 0))
      return fail(h, FILM_ERR_INVALID, "flow_filters[%d]=%d unsupported (need 32 or a multiple of 64)", i, nf);
    if (c.flow_convs[i] < 1) return fail(h, FILM_ERR_INVALID, "flow_convs[%d] must be >= 1", i);
  }
  return FILM_OK;
}

// ---------------------------------------------------------------------------------------------
// Layer table + packing
// ---------------------------------------------------------------------------------------------
std::vector<int> identity_perm(int n) {
  std::vector<int> p(n);
  for (int i = 0; i < n; ++i) p[i] = i;
  return p;
}
// internal channel order of an aligned-pyramid level: [feat0 C | feat1 C | img0 3 | img1 3 | bflow 2 | fflow 2 | 0 x6]
// reference order (interpolator.py:167-183):          [img0 3 | feat0 C | img1 3 | feat1 C | bflow 2 | fflow 2]
std::vector<int> aligned_perm(int C) {
  std::vector<int> p;
  for (int c = 0; c < C; ++c) p.push_back(3 + c);
  for (int c = 0; c < C; ++c) p.push_back(3 + C + 3 + c);
  for (int j = 0; j < 3; ++j) p.push_back(j);
  for (int j = 0; j < 3; ++j) p.push_back(3 + C + j);
  for (int j = 0; j < 4; ++j) p.push_back(2 * (3 + C) + j);
  for (int j = 0; j < 6; ++j) p.push_back(-1);
  return p;
}

// ---- Weight layouts: the transforms, the fill function of every copy, and the ONE table of the copies (kLayouts) ----
namespace {
// float -> bfloat16, round to nearest even (what v_cvt_pk_bf16_f32 does; weights are finite)
inline uint16_t bf16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// x as N bf16 planes (hi, mid[, lo]) `stride` apart: each the nearest bf16 of what the planes before it leave of x (conv_split4 on the device)
template <int N> inline void bf16_split(float x, uint16_t* d, int stride) {
  for (int p = 0; p < N; ++p) {
    const uint16_t b = bf16_rne(x);
    d[p * stride] = b;
    x = x - bf16_to_float(b);
  }
}
// Winograd kernel transforms of three taps g0 g1 g2, the results `stride` apart: F(4,3) -> 6 values, F(2,3) -> 4 values
inline void wino43_taps(float g0, float g1, float g2, float* u, int stride) {
  const float e = g0 * (1.f / 24.f) + g2 * (1.f / 6.f), o = g1 * (1.f / 12.f);
  u[0] = g0 * 0.25f;
  u[stride] = -((g0 + g2) + g1) * (1.f / 6.f);
  u[2 * stride] = -((g0 + g2) - g1) * (1.f / 6.f);
  u[3 * stride] = e + o; u[4 * stride] = e - o;
  u[5 * stride] = g2;
}
inline void wino23_taps(float g0, float g1, float g2, float* u, int stride) {
  u[0] = g0; u[stride] = ((g0 + g2) + g1) * 0.5f; u[2 * stride] = ((g0 + g2) - g1) * 0.5f; u[3 * stride] = g2;
}
// The HWIO row (`cout` contiguous floats) of kernel tap `tap` and INTERNAL input channel ci; nullptr: a zero (padding) channel
inline const float* hwio_row(const LayerPack& L, const float* src, int tap, size_t ci) {
  const int ref = L.perm[ci];
  return ref < 0 ? nullptr : src + ((size_t)tap * L.cin + ref) * L.cout;
}
inline float at(const float* row, int co) { return row ? row[co] : 0.f; }

// The three walks over a K-major layer that the copies share.  Each hands f weights of ONE output channel co in [co0, co1): an output
// channel owns disjoint ranges of every copy, which lets the packing threads share the blob.  f(co, tap, kc, v): the 16 weights of kernel tap
// `tap`, input channels [16 kc, 16 kc + 16) - the 16 source rows stay in L1 while every output channel receives its 16 k values
template <class F> void for_each_k16(const LayerPack& L, const float* src, int co0, int co1, F f) {
  for (int tap = 0; tap < L.kh * L.kw; ++tap)
    for (size_t kc = 0; kc < (size_t)L.ctot() / 16; ++kc) {
      const float* rows[16];
      for (int j = 0; j < 16; ++j) rows[j] = hwio_row(L, src, tap, kc * 16 + j);
      for (int co = co0; co < co1; ++co) {
        float v[16];
        for (int j = 0; j < 16; ++j) v[j] = at(rows[j], co);
        f(co, tap, kc, v);
      }
    }
}
// f(co, dy, kc, g): g[dx][j] = the three taps of kernel row dy of a 3x3 layer, input channels [8 kc, 8 kc + 8)
template <class F> void for_each_row_k8(const LayerPack& L, const float* src, int co0, int co1, F f) {
  for (int dy = 0; dy < 3; ++dy)
    for (size_t kc = 0; kc < (size_t)L.ctot() / 8; ++kc) {
      const float* rows[3][8];
      for (int dx = 0; dx < 3; ++dx)
        for (int j = 0; j < 8; ++j) rows[dx][j] = hwio_row(L, src, dy * 3 + dx, kc * 8 + j);
      for (int co = co0; co < co1; ++co) {
        float g[3][8];
        for (int dx = 0; dx < 3; ++dx)
          for (int j = 0; j < 8; ++j) g[dx][j] = at(rows[dx][j], co);
        f(co, dy, kc, g);
      }
    }
}
// Sub-pixel phases of upsample + 2x2.  f(co, ci, py, px, a, b, w): w = the weight of output phase (py, px) for the low-resolution tap
// (a, b), a <= py, b <= px = the kernel taps (dy, dx) that read that pixel, (py & dy) == a and (px & dx) == b, summed in raster order.
// Padding channels are skipped: their weights stay zero.
template <class F> void for_each_fold_weight(const LayerPack& L, const float* src, int co0, int co1, F f) {
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px)
      for (int a = 0; a <= py; ++a)
        for (int b = 0; b <= px; ++b)
          for (int ci = 0; ci < L.ctot(); ++ci) {
            const float* rows[4];
            for (int tp = 0; tp < 4; ++tp) rows[tp] = hwio_row(L, src, tp, ci);
            if (!rows[0]) continue;
            for (int co = co0; co < co1; ++co) {
              float acc = 0.f;
              for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx)
                  if ((py & dy) == a && (px & dx) == b) acc += rows[dy * 2 + dx][co];
              f(co, ci, py, px, a, b, acc);
            }
          }
}

// ---- the fill functions: output channels [co0, co1) of one copy (dst = its first float) from the HWIO kernel (bias: from the bias).
// The copies that are not per-channel (first layer, 1x1 heads, bias) are packed once, by the caller of co0 == 0.
void fill_bias(const LayerPack& L, const float*, const float* bias, float* dst, int co0, int) { if (co0 == 0) memcpy(dst, bias, sizeof(float) * L.cout); }
// K-major [Cout][kh*kw*ctot], k = tap * ctot + channel.  First layer: [12 tap slots][4][Cout], 1x1 heads: [ctot][Cout] - whole rows
void fill_w(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const int ct = L.ctot();
  if (L.kmajor()) {
    const size_t ktot = (size_t)L.kh * L.kw * ct;
    for_each_k16(L, src, co0, co1, [&](int co, int tap, size_t kc, const float* v) { memcpy(dst + (size_t)co * ktot + (size_t)tap * ct + kc * 16, v, 16 * sizeof(float)); });
  } else if (co0 == 0) {
    for (int tap = 0; tap < L.kh * L.kw; ++tap)
      for (int ci = 0; ci < ct; ++ci)
        if (const float* row = hwio_row(L, src, tap, ci)) memcpy(dst + ((size_t)tap * (L.c3 ? 4 : ct) + ci) * L.cout, row, sizeof(float) * L.cout);
  }
}
// conv_halo_kernel: [Cout][ctot/16][9][16]
void fill_wh(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nkc = (size_t)L.ctot() / 16;
  for_each_k16(L, src, co0, co1, [&](int co, int tap, size_t kc, const float* v) { memcpy(dst + (((size_t)co * nkc + kc) * 9 + tap) * 16, v, 16 * sizeof(float)); });
}
// conv_halo_split_kernel: the same cells as three bf16 planes, [Cout][ctot/16][9][3][16] bf16
void fill_ws(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nkc = (size_t)L.ctot() / 16;
  for_each_k16(L, src, co0, co1, [&](int co, int tap, size_t kc, const float* v) {
    uint16_t* d = reinterpret_cast<uint16_t*>(dst) + (((size_t)co * nkc + kc) * 9 + tap) * 48;
    for (int j = 0; j < 16; ++j) bf16_split<3>(v[j], d + j, 16);
  });
}
// the four phases one behind the other, phase (py, px): [Cout][ntaps * ctot], tap t = a * (px + 1) + b; 1 + 2 + 2 + 4 = 9 taps in all
void fill_wf(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t ct = L.ctot();
  for_each_fold_weight(L, src, co0, co1, [&](int co, int ci, int py, int px, int a, int b, float w) {
    static const int kTapsBefore[4] = {0, 1, 3, 5};
    dst[(kTapsBefore[py * 2 + px] * L.cout + (size_t)co * (py + 1) * (px + 1) + a * (px + 1) + b) * ct + ci] = w;
  });
}
// conv_foldx3_kernel: the phase weights as bf16 hi / mid, [Cout][ctot/16][9 (tap, phase) steps][plane][16] bf16
void fill_wfx(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nkc = (size_t)L.ctot() / 16;
  // step of (tap a*2+b, phase py*2+px) in the kernel's order (taps 00 00 00 | 00 01 01 | 10 10 11)
  static const int kFoldStep[4][4] = {{0, 1, 2, 3}, {-1, 4, -1, 5}, {-1, -1, 6, 7}, {-1, -1, -1, 8}};
  for_each_fold_weight(L, src, co0, co1, [&](int co, int ci, int py, int px, int a, int b, float w) {
    bf16_split<2>(w, reinterpret_cast<uint16_t*>(dst) + (((size_t)co * nkc + ci / 16) * 9 + kFoldStep[a * 2 + b][py * 2 + px]) * 32 + ci % 16, 16);
  });
}
// conv_fold4_kernel, the difference form of upsample + 2x2: [Cout/32][ctot/8][plane 4][K half][32][4], planes S = ((W00 + W01) + W10) + W11,
// Sx = W01 + W11, Sy = W10 + W11, W11 (padding channels: zero rows)
void fill_wf4(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nk8 = (size_t)L.ctot() / 8;
  for (int ci = 0; ci < L.ctot(); ++ci) {
    const float* rows[4];
    for (int tp = 0; tp < 4; ++tp) rows[tp] = hwio_row(L, src, tp, ci);
    for (int co = co0; co < co1; ++co) {
      const float w[4] = {at(rows[0], co), at(rows[1], co), at(rows[2], co), at(rows[3], co)};
      const float pl[4] = {((w[0] + w[1]) + w[2]) + w[3], w[1] + w[3], w[2] + w[3], w[3]};
      for (int q = 0; q < 4; ++q)
        dst[((((size_t)(co / 32) * nk8 + ci / 8) * 4 + q) * 2 + (ci % 8) / 4) * 128 + (co % 32) * 4 + ci % 4] = pl[q];
    }
  }
}
// conv_wino43_kernel: F(4,3) along x, [Cout][ctot/8][3 dy][6 nu][8]
void fill_w43(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nk8 = (size_t)L.ctot() / 8;
  for_each_row_k8(L, src, co0, co1, [&](int co, int dy, size_t kc, const float (*g)[8]) {
    for (int j = 0; j < 8; ++j) wino43_taps(g[0][j], g[1][j], g[2][j], dst + (((size_t)co * nk8 + kc) * 3 + dy) * 48 + j, 8);
  });
}
// conv_wino_kernel: F(2,3) along x, [Cout][ctot/8][nu * 3 + dy][8]
void fill_ww(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nk8 = (size_t)L.ctot() / 8;
  for_each_row_k8(L, src, co0, co1, [&](int co, int dy, size_t kc, const float (*g)[8]) {
    for (int j = 0; j < 8; ++j) wino23_taps(g[0][j], g[1][j], g[2][j], dst + (((size_t)co * nk8 + kc) * 12 + dy) * 8 + j, 24);
  });
}
// conv_winox3_kernel: the same transformed weights as bf16 hi / mid, [Cout][ctot/16][dy][j][h][plane][16] bf16 (nu = 2h + j)
void fill_wx(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nk16 = (size_t)L.ctot() / 16;
  for_each_row_k8(L, src, co0, co1, [&](int co, int dy, size_t kc, const float (*g)[8]) {
    float u[4][8];
    for (int j = 0; j < 8; ++j) wino23_taps(g[0][j], g[1][j], g[2][j], &u[0][j], 8);
    for (int nu = 0; nu < 4; ++nu) {
      uint16_t* d = reinterpret_cast<uint16_t*>(dst) + ((((size_t)co * nk16 + kc / 2) * 3 + dy) * 2 + (nu & 1)) * 64 + (nu >> 1) * 32 + (kc & 1) * 8;
      for (int j = 0; j < 8; ++j) bf16_split<2>(u[nu][j], d + j, 16);
    }
  });
}
// conv_wino2d_kernel: U[mu][nu] = F(2,3) along dy of the F(4,3)-along-dx transformed kernel rows (the u of the w43 copy),
// [Cout/32][ctot/8][mu 4][nu 6][K half][32][4]
void fill_w2d(const LayerPack& L, const float* src, const float*, float* dst, int co0, int co1) {
  const size_t nk8 = (size_t)L.ctot() / 8;
  for (size_t kc = 0; kc < nk8; ++kc) {
    const float* rows[9][8];
    for (int tap = 0; tap < 9; ++tap)
      for (int j = 0; j < 8; ++j) rows[tap][j] = hwio_row(L, src, tap, kc * 8 + j);
    for (int co = co0; co < co1; ++co)
      for (int j = 0; j < 8; ++j) {
        float u[3][6], U[4];
        for (int dy = 0; dy < 3; ++dy) wino43_taps(at(rows[dy * 3][j], co), at(rows[dy * 3 + 1][j], co), at(rows[dy * 3 + 2][j], co), u[dy], 1);
        for (int nu = 0; nu < 6; ++nu) {
          wino23_taps(u[0][nu], u[1][nu], u[2][nu], U, 1);
          for (int mu = 0; mu < 4; ++mu)
            dst[(((((size_t)(co / 32) * nk8 + kc) * 4 + mu) * 6 + nu) * 2 + j / 4) * 128 + (co % 32) * 4 + j % 4] = U[mu];
        }
      }
  }
}

// THE table of weight layouts: one row per copy of a layer's weights in the packed blob.  The copies lie in four contiguous GROUPS, packed
// and uploaded on demand (film_finalize: what the options need at once; the planner: the group of the copy a kernel family reads,
// layout_groups, when a plan first needs it), so that the default fp32 path neither builds nor broadcasts the copies it never reads:
//   0 = what the default plan runs on: K-major / first-layer / 1x1 layouts + biases, both forms of the upsample + 2x2 layers, the F(4,3)
//       and nested Winograd copies (3.1x the parameters);  1 = F(2,3) copy (conv_wino_kernel: levels narrower than the F(4,3) patches);
//   2 = halo copy (conv_halo_kernel: option winograd = 0 / halo_all);  3 = bf16 split copies (precision modes bf16x6 / bf16x3).
// Within a group the copies follow each other layer by layer, within a layer in row order, each from a multiple of four floats.  Offsets
// are an external format (plan JSON); tests/plan_interp.py restates every layout independently.
struct WeightLayout {
  int64_t LayerPack::* off;                // receives the copy's offset in the blob (floats; -1: the layer has no such copy)
  int group;
  bool (LayerPack::*has)() const;          // the layers that have the copy; nullptr: all
  int64_t (*floats)(const LayerPack&);
  void (*fill)(const LayerPack& L, const float* kernel, const float* bias, float* dst, int co0, int co1);
  bool on(const LayerPack& L) const { return !has || (L.*has)(); }
};
int64_t weights_of(const LayerPack& L) { return (int64_t)L.ctot() * L.cout; }   // per kernel tap
const WeightLayout kLayouts[] = {
  {&LayerPack::w_off, 0, nullptr, [](const LayerPack& L) { return L.packed_rows() * L.cout; }, fill_w},
  {&LayerPack::b_off, 0, nullptr, [](const LayerPack& L) { return (int64_t)L.cout; }, fill_bias},
  {&LayerPack::wf_off, 0, &LayerPack::has_fold, [](const LayerPack& L) { return 9 * weights_of(L); }, fill_wf},
  {&LayerPack::wf4_off, 0, &LayerPack::has_fold4, [](const LayerPack& L) { return 4 * weights_of(L); }, fill_wf4},
  {&LayerPack::w43_off, 0, &LayerPack::has_halo, [](const LayerPack& L) { return 3 * 6 * weights_of(L); }, fill_w43},
  {&LayerPack::w2d_off, 0, &LayerPack::has_w2d, [](const LayerPack& L) { return 4 * 6 * weights_of(L); }, fill_w2d},
  {&LayerPack::ww_off, 1, &LayerPack::has_halo, [](const LayerPack& L) { return 3 * 4 * weights_of(L); }, fill_ww},
  {&LayerPack::wh_off, 2, &LayerPack::has_halo, [](const LayerPack& L) { return 9 * weights_of(L); }, fill_wh},
  {&LayerPack::wfx_off, 3, &LayerPack::has_fold, [](const LayerPack& L) { return 9 * weights_of(L); }, fill_wfx},               // 2 bf16 = 1 float
  {&LayerPack::ws_off, 3, &LayerPack::has_halo, [](const LayerPack& L) { return (9 * weights_of(L) * 3 + 1) / 2; }, fill_ws},   // 3 bf16 = 1.5
  {&LayerPack::wx_off, 3, &LayerPack::has_halo, [](const LayerPack& L) { return 3 * 4 * weights_of(L); }, fill_wx},
};
}  // namespace

int layout_groups(int64_t ConvWeights::* copy) {
  for (const WeightLayout& r : kLayouts)
    if (r.off == static_cast<int64_t LayerPack::*>(copy)) return r.group + 1;
  return 1;
}

void build_layers(film_t* h) {
  const film_config& c = h->cfg;
  h->layers.clear();
  h->layer_idx.clear();
  auto add = [&](const std::string& name, int kh, int kw, int cin, int cout, std::vector<int> perm) {
    LayerPack L;
    L.name = name; L.kh = kh; L.kw = kw; L.cin = cin; L.cout = cout; L.perm = std::move(perm);
    h->layer_idx[name] = (int)h->layers.size();
    h->layers.push_back(std::move(L));
  };
  int cin = 3;
  for (int i = 0; i < c.sub_levels; ++i) {
    int k = c.filters << i;
    add("feat_net/sub_extractor/cfeat_conv_" + std::to_string(2 * i), 3, 3, cin, k, identity_perm(cin));
    if (i == 0) h->layers.back().c3 = true;
    add("feat_net/sub_extractor/cfeat_conv_" + std::to_string(2 * i + 1), 3, 3, k, k, identity_perm(k));
    cin = k;
  }
  auto fc = feature_channels(c);
  for (int p = 0; p <= c.specialized_levels; ++p) {
    std::string prefix = predictor_prefix(c, p);
    int ci = 2 * fc[std::min(p, c.pyramid_levels - 1)];
    int nf = c.flow_filters[p], nconv = c.flow_convs[p];
    for (int j = 0; j < nconv; ++j) {
      add(prefix + "/conv_" + std::to_string(j), 3, 3, ci, nf, identity_perm(ci));
      ci = nf;
    }
    add(prefix + "/conv_" + std::to_string(nconv), 1, 1, nf, nf / 2, identity_perm(nf));
    add(prefix + "/conv_" + std::to_string(nconv + 1), 1, 1, nf / 2, 2, identity_perm(nf / 2));
  }
  auto ff = fusion_filters(c);
  const int FL = c.fusion_pyramid_levels;
  for (int i = 0; i < FL - 1; ++i) {
    const int aligned_ref = 2 * (3 + fc[i]) + 4;
    std::vector<int> p0;
    int net_c;
    if (i == FL - 2) { net_c = 2 * (3 + fc[FL - 1]) + 4; p0 = aligned_perm(fc[FL - 1]); }
    else { net_c = ff[i + 1]; p0 = identity_perm(net_c); }
    add("fusion/convs_" + std::to_string(i) + "_0", 2, 2, net_c, ff[i], p0);
    std::vector<int> p1 = aligned_perm(fc[i]);
    for (int j = 0; j < ff[i]; ++j) p1.push_back(aligned_ref + j);
    add("fusion/convs_" + std::to_string(i) + "_1", 3, 3, aligned_ref + ff[i], ff[i], p1);
    add("fusion/convs_" + std::to_string(i) + "_2", 3, 3, ff[i], ff[i], identity_perm(ff[i]));
  }
  add("fusion/output_conv", 1, 1, ff[0], 3, identity_perm(ff[0]));
  // offsets: group by group, layer by layer, in the order of the table's rows
  int64_t off = 0;
  for (int g = 0; g < 4; ++g) {
    for (auto& L : h->layers)
      for (const WeightLayout& r : kLayouts)
        if (r.group == g && r.on(L)) { L.*r.off = off; off = (off + r.floats(L) + 3) & ~int64_t(3); }
    h->group_end[g] = off;
  }
  h->packed_floats = 0;
  h->groups_packed = 0;
}

}  // namespace film_internal

using namespace film_internal;

extern "C" {

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), slicing-by-8.  Host-side helper of the SavedModel
// variables reader (film_hip/tf_bundle.py): TensorFlow stores a masked crc32c per tensor and per index block.
uint32_t film_crc32c(uint32_t crc, const void* data, int64_t n) {
  static uint32_t tab[8][256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      tab[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int t = 1; t < 8; ++t) tab[t][i] = (tab[t - 1][i] >> 8) ^ tab[0][tab[t - 1][i] & 0xFF];
    init = true;
  }
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint32_t c = ~crc;
  while (n > 0 && (reinterpret_cast<uintptr_t>(p) & 7)) { c = tab[0][(c ^ *p++) & 0xFF] ^ (c >> 8); --n; }
  while (n >= 8) {
    uint64_t v;
    memcpy(&v, p, 8);
    v ^= c;
    c = tab[7][v & 0xFF] ^ tab[6][(v >> 8) & 0xFF] ^ tab[5][(v >> 16) & 0xFF] ^ tab[4][(v >> 24) & 0xFF] ^
        tab[3][(v >> 32) & 0xFF] ^ tab[2][(v >> 40) & 0xFF] ^ tab[1][(v >> 48) & 0xFF] ^ tab[0][(v >> 56) & 0xFF];
    p += 8; n -= 8;
  }
  while (n-- > 0) c = tab[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
  return ~c;
}

int film_set_weight(film_t* h, const char* name, const float* data, const int64_t* dims, int ndim) {
  if (!h || !name || !data || !dims || ndim < 1 || ndim > 4) return fail(h, FILM_ERR_INVALID, "bad argument");
  std::string nm(name);
  const size_t slash = nm.rfind('/');
  if (slash == std::string::npos) return fail(h, FILM_ERR_NOTFOUND, "unknown weight '%s'", name);
  const std::string layer = nm.substr(0, slash), kind = nm.substr(slash + 1);
  auto it = h->layer_idx.find(layer);
  if (it == h->layer_idx.end() || (kind != "kernel" && kind != "bias")) return fail(h, FILM_ERR_NOTFOUND, "unknown weight '%s'", name);
  const LayerPack& L = h->layers[it->second];
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= dims[i];
  if (kind == "kernel") {
    if (ndim != 4 || dims[0] != L.kh || dims[1] != L.kw || dims[2] != L.cin || dims[3] != L.cout)
      return fail(h, FILM_ERR_INVALID, "%s: expected HWIO [%d,%d,%d,%d]", name, L.kh, L.kw, L.cin, L.cout);
  } else if (ndim != 1 || dims[0] != L.cout) {
    return fail(h, FILM_ERR_INVALID, "%s: expected [%d]", name, L.cout);
  }
  HostTensor t;
  t.dims.assign(dims, dims + ndim);
  t.data.assign(data, data + n);
  h->host_w[nm] = std::move(t);
  h->finalized = false;
  return FILM_OK;
}

// Uploads the floats [from, to) of the packed blob.  The device buffer is sized for every layout group once (1.1 GB of
// 288): groups packed later land at their fixed offsets and no plan has to be rebuilt.
static int upload_packed(film_t* h, int64_t from, int64_t to) {
  if (h->plan_only || to <= from) return FILM_OK;
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->packed_dev) HIPCHK(h, hipMalloc(&h->packed_dev, (size_t)h->group_end[3] * sizeof(float)));
  HIPCHK(h, hipMemcpy(h->packed_dev + from, h->packed_host.data() + from, (size_t)(to - from) * sizeof(float), hipMemcpyHostToDevice));
  return FILM_OK;
}

// Packs layout groups [h->groups_packed, n) from the HWIO tensors (kept on the host) and uploads them.  Work items =
// (layer, 32 output channels), pulled from an atomic counter by up to 32 threads: 137.7 MB of parameters into the
// default group 0 in well under a second on the hosts this runs on (it took 7 s single-threaded for every layout).
int film_ensure_groups_(film_t* h, int n) {
  if (n <= h->groups_packed) return FILM_OK;
  if (n > 4) n = 4;
  for (const LayerPack& L : h->layers)
    if (!h->host_w.count(L.name + "/kernel") || !h->host_w.count(L.name + "/bias")) return fail(h, FILM_ERR_STATE, "missing weight '%s'", L.name.c_str());
  const int64_t from = h->groups_packed ? h->group_end[h->groups_packed - 1] : 0, to = h->group_end[n - 1];
  h->packed_host.resize((size_t)to, 0.f);
  struct Item { const LayerPack* L; const float *kernel, *bias; int co0, co1; };
  std::vector<Item> items;
  for (const LayerPack& L : h->layers)
    for (int co = 0; co < L.cout; co += 32)
      items.push_back({&L, h->host_w.at(L.name + "/kernel").data.data(), h->host_w.at(L.name + "/bias").data.data(), co, std::min(L.cout, co + 32)});
  for (int g = h->groups_packed; g < n; ++g) {
    std::atomic<size_t> next{0};
    auto worker = [&]() {   // an item: every copy of group g that the layer has, for the item's output channels
      for (size_t i; (i = next.fetch_add(1)) < items.size();) {
        const Item& it = items[i];
        for (const WeightLayout& r : kLayouts)
          if (r.group == g && r.on(*it.L)) r.fill(*it.L, it.kernel, it.bias, h->packed_host.data() + it.L->*r.off, it.co0, it.co1);
      }
    };
    const unsigned nth = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nth; ++t) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
  }
  h->groups_packed = n;
  h->packed_floats = to;
  return upload_packed(h, from, to);
}

// layout groups the current options need at once (the planner asks for more when a plan needs them)
static int groups_for_options(const film_t* h) {
  int n = 1;
  auto runs = [&](ConvFamily f) { n = std::max(n, layout_groups(kConvFamily[f].weights)); };
  if (h->opt_wino == 2) runs(FAM_WINO);
  if (h->opt_wino == 0 || h->opt_halo_all) runs(FAM_HALO);
  if (h->opt_precision) runs(FAM_SPLIT6);
  return n;
}

int film_finalize(film_t* h) {
  if (!h) return FILM_ERR_INVALID;
  // A handle that has already run may hold cached plans whose ops point into layout groups 1..3 (F(2,3), halo, bf16
  // copies pulled in by Planner::need_groups).  A second weight set must reach those regions too, or such a plan
  // would mix the new group-0 layouts with the previous set's copies: re-pack everything that was packed before.
  const int prev = h->groups_packed;
  h->groups_packed = 0;
  h->packed_floats = 0;
  h->packed_host.clear();
  h->finalized = false;
  if (!h->plan_only && prev > 0) {   // replays of the previous weight set may still be in flight on the caller's stream
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
  }
  int rc = film_ensure_groups_(h, std::max(groups_for_options(h), prev));
  if (rc) return rc;
  h->finalized = true;
  return FILM_OK;
}

// ---- the parameter set as ONE flat blob (what ranks exchange): per layer, in layer order, the HWIO kernel then the bias ----
static int64_t flat_floats(const film_t* h) {
  int64_t n = 0;
  for (const LayerPack& L : h->layers) n += (int64_t)L.kh * L.kw * L.cin * L.cout + L.cout;
  return n;
}

int film_packed_size(film_t* h, int64_t* n) {
  if (!h || !n) return FILM_ERR_INVALID;
  *n = flat_floats(h);
  return FILM_OK;
}

int film_export_packed(film_t* h, float* dst, int64_t cap, int mem_kind) {
  if (!h || !dst) return FILM_ERR_INVALID;
  if (!h->finalized) return fail(h, FILM_ERR_STATE, "film_finalize has not been called");
  const int64_t n = flat_floats(h);
  if (cap < n) return fail(h, FILM_ERR_INVALID, "capacity %lld < %lld floats", (long long)cap, (long long)n);
  std::vector<float> tmp;
  float* out = dst;
  if (mem_kind != FILM_MEM_HOST) {
    if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle has no device");
    tmp.resize((size_t)n);
    out = tmp.data();
  }
  int64_t off = 0;
  for (const LayerPack& L : h->layers) {
    const HostTensor& k = h->host_w.at(L.name + "/kernel");
    const HostTensor& bq = h->host_w.at(L.name + "/bias");
    memcpy(out + off, k.data.data(), k.data.size() * sizeof(float)); off += (int64_t)k.data.size();
    memcpy(out + off, bq.data.data(), bq.data.size() * sizeof(float)); off += (int64_t)bq.data.size();
  }
  if (mem_kind != FILM_MEM_HOST) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(dst, tmp.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  }
  return FILM_OK;
}

int film_import_packed(film_t* h, const float* src, int64_t n, int mem_kind) {
  if (!h || !src) return FILM_ERR_INVALID;
  if (n != flat_floats(h)) return fail(h, FILM_ERR_INVALID, "blob has %lld floats, expected %lld", (long long)n, (long long)flat_floats(h));
  std::vector<float> tmp;
  const float* in = src;
  if (mem_kind != FILM_MEM_HOST) {
    if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle has no device");
    tmp.resize((size_t)n);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(tmp.data(), src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    in = tmp.data();
  }
  int64_t off = 0;
  for (const LayerPack& L : h->layers) {
    HostTensor k, bq;
    k.dims = {L.kh, L.kw, L.cin, L.cout};
    k.data.assign(in + off, in + off + (int64_t)L.kh * L.kw * L.cin * L.cout); off += (int64_t)k.data.size();
    bq.dims = {L.cout};
    bq.data.assign(in + off, in + off + L.cout); off += L.cout;
    h->host_w[L.name + "/kernel"] = std::move(k);
    h->host_w[L.name + "/bias"] = std::move(bq);
  }
  return film_finalize(h);
}

// ---- RCCL weight broadcast (include/film_hip.h).  ncclBroadcast is looked up at run time: a process has ONE RCCL (PyTorch bundles its own),
// and a host that brings a communicator has it loaded already.
namespace {
typedef int (*nccl_bcast_fn)(const void*, void*, size_t, int /* ncclDataType_t */, int, void* /* ncclComm_t */, hipStream_t);
nccl_bcast_fn resolve_nccl_broadcast(std::string* where) {
  if (void* f = dlsym(RTLD_DEFAULT, "ncclBroadcast")) { *where = "the process"; return reinterpret_cast<nccl_bcast_fn>(f); }
  for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
    if (void* lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))
      if (void* f = dlsym(lib, "ncclBroadcast")) { *where = name; return reinterpret_cast<nccl_bcast_fn>(f); }
  }
  return nullptr;
}
}  // namespace

int film_bcast_weights(film_t* h, void* nccl_comm, int root, int rank, void* stream) {
  if (!h || !nccl_comm || root < 0 || rank < 0) return fail(h, FILM_ERR_INVALID, "bad argument");
  if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle: the RCCL broadcast needs a HIP device");
  if (rank == root && !h->finalized) return fail(h, FILM_ERR_STATE, "the root rank must hold a finalized weight set (film_finalize / film_load_bundle)");
  static std::string where;
  static const nccl_bcast_fn bcast = resolve_nccl_broadcast(&where);
  if (!bcast) return fail(h, FILM_ERR_NOTFOUND, "ncclBroadcast not found: no RCCL in the process and librccl.so cannot be loaded");
  const int64_t n = flat_floats(h);
  HIPCHK(h, hipSetDevice(h->device));
  float* blob = nullptr;
  HIPCHK(h, hipMalloc(&blob, (size_t)n * sizeof(float)));
  hipStream_t s = stream ? (hipStream_t)stream : h->stream;
  int rc = FILM_OK;
  if (rank == root) rc = film_export_packed(h, blob, n, FILM_MEM_DEVICE);
  if (rc == FILM_OK) {
    const int nrc = bcast(blob, blob, (size_t)n, 7 /* ncclFloat32 */, root, nccl_comm, s);
    if (nrc != 0) rc = fail(h, FILM_ERR_HIP, "ncclBroadcast (from %s) failed with ncclResult_t %d", where.c_str(), nrc);
  }
  if (rc == FILM_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(h, FILM_ERR_HIP, "hipStreamSynchronize behind the broadcast failed: %s", hipGetErrorString(hipGetLastError()));
  if (rc == FILM_OK && rank != root) rc = film_import_packed(h, blob, n, FILM_MEM_DEVICE);
  (void)hipFree(blob);
  return rc;
}

// the kernel-layout blob (debug / tests): the packed prefix [0, *n)
int film_export_layouts(film_t* h, float* dst, int64_t cap, int64_t* n) {
  if (!h) return FILM_ERR_INVALID;
  if (!h->finalized) return fail(h, FILM_ERR_STATE, "film_finalize has not been called");
  if (n) *n = h->packed_floats;
  if (!dst) return FILM_OK;
  if (cap < h->packed_floats) return fail(h, FILM_ERR_INVALID, "capacity %lld < %lld floats", (long long)cap, (long long)h->packed_floats);
  memcpy(dst, h->packed_host.data(), (size_t)h->packed_floats * sizeof(float));
  return FILM_OK;
}

}  // extern "C"
