// film_tune.cpp -- the tile shapes a convolution op may run on (the candidates of each kernel family, kConvFamily in film_kernels.h), the
// per-shape autotuner that times them once per plan, and the tune cache as text (film_export_tune / film_import_tune).
#include "film_internal.h"

namespace film_internal {
namespace {
// every shape with and without the XCD-contiguous block mapping
std::vector<int> both_maps(ConvFamily f, const std::vector<int>& shapes) {
  std::vector<int> out;
  for (int sh : shapes) { out.push_back(conv_tile(f, sh, false)); out.push_back(conv_tile(f, sh, true)); }
  return out;
}

std::string conv_signature(const OpDesc& op) {
  std::ostringstream o;
  const FamilyCodes fc = family_codes(op.family);
  o << op.NB << 'x' << op.H << 'x' << op.W << ':' << op.Cout << ':' << op.ksize << ':' << op.out.stride << ':' << fc.c3 << ':' << fc.halo << ':' << fc.split << ':' << fc.wino << ':' << op.fold << ':' << op.ksplit << ':' << (op.out2.buf >= 0) << ':' << op.pw_cout;
  for (int i = 0; i < op.nseg; ++i)
    o << '|' << op.seg[i].v.C << ',' << op.seg[i].v.stride << ',' << op.seg[i].up << ',' << op.seg[i].bmod;
  return o.str();
}
}  // namespace

std::vector<int> tile_candidates(const OpDesc& op) {
  if (op.Cout % 128 == 0) return both_maps(FAM_BUF, {TILE_128x128, TILE_256x128, TILE_256x64, TILE_128x64, TILE_64x64});
  if (op.Cout % 64 == 0) return both_maps(FAM_BUF, {TILE_256x64, TILE_128x64, TILE_64x64, TILE_256x32, TILE_128x32});
  return both_maps(FAM_BUF, {TILE_256x32, TILE_128x32});
}

// the 3-channel first layer has one kernel (conv_c3_kernel)
std::vector<int> c3_candidates(const OpDesc&) { return {conv_tile(FAM_C3, TILE_C3_DIRECT, false)}; }

// conv_halo_kernel, and the same shapes on conv_halo_split_kernel (bf16x6 / bf16x3)
std::vector<int> halo_candidates(const OpDesc& op) {
  if (op.Cout % 128 == 0) return both_maps(op.family, {HALO_4x64, HALO_4x128, HALO_8x64, HALO_8x128});
  if (op.Cout % 64 == 0) return both_maps(op.family, {HALO_4x64, HALO_8x64, HALO_4x32, HALO_8x32});
  return both_maps(op.family, {HALO_8x32, HALO_4x32});
}

std::vector<int> wino_candidates(const OpDesc& op) {
  if (op.Cout % 128 == 0) return both_maps(FAM_WINO, {WINO_4x64_W8, WINO_8x64_W16, WINO_2x64, WINO_4x128_W16, WINO_4x128});
  if (op.Cout % 64 == 0) return both_maps(FAM_WINO, {WINO_4x64_W8, WINO_8x64_W16, WINO_2x64, WINO_4x32});
  return both_maps(FAM_WINO, {WINO_4x32, WINO_8x32_W8});
}

std::vector<int> wino43_candidates(const OpDesc& op) {
  const bool pool = op.out2.buf >= 0, pw = op.pw_out.buf >= 0;
  std::vector<int> shapes;
  if (pw)   // the fused 1x1 needs every channel of a pixel in one workgroup: the NH = 1 tiles at Cout = 64
    shapes = {W43_Q16_4x64_N1, W43_Q16_4x64_N1_P2, W43_Q8_8x64_N1_P2};
  // the 64-pixel ("Q16", two workgroups per CU) tiles won every layer of the 1080p plan against the 128-pixel ones
  // (profiles/r02_conv_bench_w43.log); one 128-pixel tile stays in the list for shapes nobody measured.  The 32-pixel x
  // 8-row ("Q8") tiles win on the 480-wide level (15 patches per row exactly: -3..5 %) and, with 32 channels and the weight
  // ring (three workgroups per CU), on the 128 -> 32 layer of flow level 0 (-7 %): profiles/r03_conv_bench_w43.log
  else if (op.Cout % 64 == 0)
    shapes = {W43_4x64_T21, W43_Q16_4x64_T21, W43_Q16_4x64_T12, W43_Q16_4x32_T11, W43_Q16_4x64_N1,
              W43_Q16_4x64_T21_P2, W43_Q16_4x64_T12_P2, W43_Q16_4x32_T11_P2, W43_Q16_4x64_N1_P2, W43_Q16_4x32_T11_BG,
              W43_Q8_8x64_T21_P2, W43_Q8_8x64_T12_P2, W43_Q8_8x64_N1_P2, W43_Q8_8x32_T11_BG, W43_Q8_8x32_T11_P2};
  else
    shapes = {W43_4x32_T11, W43_Q16_4x32_T11, W43_Q16_4x32_T11_P2, W43_Q16_4x32_T11_BG, W43_Q8_8x32_T11_BG, W43_Q8_8x32_T11_P2};
  std::vector<int> keep;
  for (int sh : shapes) {
    if (!film_w43_shape_built(sh)) continue;   // (the default library holds seven of the seventeen tiles)
    if (pool && (sh == W43_4x64_T21 || sh == W43_4x64_T12 || sh == W43_4x32_T11)) continue;   // the fused pool needs a <= 64-pixel tile
    keep.push_back(sh);
  }
  return both_maps(FAM_W43, keep);
}

// (H, W: the level.  The square arrangement is a candidate where its tiles pad the level no more than the 8 x 32 ones.)
std::vector<int> wino2d_candidates(const OpDesc& op) {
  const int H = op.H, W = op.W;
  const bool pw = op.pw_out.buf >= 0;
  const int64_t pad_r = (int64_t)((W + 31) / 32) * ((H + 7) / 8), pad_s = (int64_t)((W + 15) / 16) * ((H + 15) / 16);
  const bool sq = pad_s <= pad_r;
  std::vector<int> shapes;
  if (pw || op.Cout % 64 == 0) { shapes.push_back(W2D_8x64); if (sq) shapes.push_back(W2D_16x64); }
  if (!pw) {   // (the fused 1x1 needs every channel of a pixel in one workgroup)
    shapes.push_back(W2D_8x32); shapes.push_back(W2D_8x32_S2);
    if (sq) { shapes.push_back(W2D_16x32); shapes.push_back(W2D_16x32_S2); }
  }
  return both_maps(FAM_W2D, shapes);
}

std::vector<int> fold4_candidates(const OpDesc& op) {
  return both_maps(FAM_FOLD4, op.Cout % 64 == 0 ? std::vector<int>{F4_4x64, F4_4x32} : std::vector<int>{F4_4x32});
}

std::vector<int> foldx3_candidates(const OpDesc& op) {
  return both_maps(FAM_FOLDX3, op.Cout % 128 == 0 ? std::vector<int>{FX3_4x64, FX3_8x64, FX3_4x128} : std::vector<int>{FX3_4x64, FX3_8x64});
}

std::vector<int> winox3_candidates(const OpDesc& op) {
  if (op.Cout % 128 == 0) return both_maps(FAM_WINOX3, {WX3_4x128_T22, WX3_4x64_T12, WX3_4x64_T21});
  if (op.Cout % 64 == 0) return both_maps(FAM_WINOX3, {WX3_4x64_T12, WX3_4x64_T21, WX3_4x32_T11});
  return both_maps(FAM_WINOX3, {WX3_4x32_T11});
}

std::vector<int> conv_candidates(const OpDesc& op) { return kConvFamily[op.family].candidates(op); }

// Measure, don't guess: every distinct conv shape of a plan is timed once with each tile shape that fits
// its Cout (random activations, the real weights) and keeps the fastest.  The choice cannot change the
// results: every output element is the same k-ordered fma chain whatever the tile.
int autotune_plan(film_t* h, Plan* P, bool measure) {
  bool need = false;
  for (const OpDesc& op : P->ops) {
    if (op.kind != OP_CONV || !measure) continue;
    const std::string sig = conv_signature(op);
    if (h->tune_cache.count(sig)) continue;
    auto it = h->tune_import.find(sig);
    if (it != h->tune_import.end()) {   // an earlier process measured this shape: keep its choice if it is still a candidate
      const std::vector<int> cands = conv_candidates(op);
      if (std::find(cands.begin(), cands.end(), it->second) != cands.end()) { h->tune_cache[sig] = it->second; continue; }
    }
    need = true;
  }
  if (need) {
    HIPCHK(h, film_launch_fill_random(P->arena, P->arena_floats, 0x9e3779b9u, h->stream));
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    for (OpDesc& op : P->ops) {
      if (op.kind != OP_CONV) continue;
      const std::string sig = conv_signature(op);
      if (h->tune_cache.count(sig)) continue;
      int best = op.tile;
      float best_ms = 1e30f;
      const std::vector<int> cands = conv_candidates(op);
      auto launch_tile = [&](int tile) -> hipError_t {
        OpDesc trial = op;
        trial.tile = tile;
        return launch_op(trial, P->arena, h->packed_dev, h->stream);
      };
      auto time_once = [&](int tile, float* ms) -> int {
        HIPCHK(h, hipEventRecord(e0, h->stream));
        HIPCHK(h, launch_tile(tile));
        HIPCHK(h, hipEventRecord(e1, h->stream));
        HIPCHK(h, hipEventSynchronize(e1));
        HIPCHK(h, hipEventElapsedTime(ms, e0, e1));
        return FILM_OK;
      };
      std::vector<std::pair<float, int>> timed;
      for (int tile : cands) {
        HIPCHK(h, launch_tile(tile));  // warm
        float ms_min = 1e30f, ms_sum = 0.f;
        // at least two timed launches; with the "tune_ms" option keep going until that much kernel time has been
        // spent on the candidate (long enough for the power-limited clock to settle)
        for (int rep = 0; rep < 2 || (ms_sum < (float)h->opt_tune_ms && rep < 64); ++rep) {
          float ms = 0;
          int trc = time_once(tile, &ms);
          if (trc) return trc;
          ms_min = std::min(ms_min, ms);
          ms_sum += ms;
        }
        timed.push_back({ms_min, tile});
      }
      // Run-off: the candidates within 6 % of the fastest (at most four) are timed four more times each, round robin, so
      // that a single lucky launch (clock state, neighbours in L2) does not decide a layer that runs every forward.
      std::sort(timed.begin(), timed.end());
      size_t nfin = 0;
      while (nfin < timed.size() && nfin < 4 && timed[nfin].first <= timed[0].first * 1.06f) ++nfin;
      if (nfin > 1)
        for (int round = 0; round < 4; ++round)
          for (size_t c = 0; c < nfin; ++c) {
            float ms = 0;
            int trc = time_once(timed[c].second, &ms);
            if (trc) return trc;
            timed[c].first = std::min(timed[c].first, ms);
          }
      for (size_t c = 0; c < std::max<size_t>(nfin, 1) && c < timed.size(); ++c)
        if (timed[c].first < best_ms) { best_ms = timed[c].first; best = timed[c].second; }
      // conv_wino2d_kernel: a 64-channel tile within 2 % of the fastest wins - it reads its input patch half as often (45.2 -> 40.2
      // GB of fabric reads per 1080p forward with the tile forced, same step time: profiles/r04_w2d_tile64_ab.log)
      if (op.family == FAM_W2D && !film_w2d_64(best & 15)) {
        float ms64 = 1e30f;
        int t64 = -1;
        for (size_t c = 0; c < std::max<size_t>(nfin, 1) && c < timed.size(); ++c)
          if (film_w2d_64(timed[c].second & 15) && timed[c].first < ms64) { ms64 = timed[c].first; t64 = timed[c].second; }
        if (t64 >= 0 && ms64 <= best_ms * 1.02f) best = t64;
      }
      h->tune_cache[sig] = best;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIPCHK(h, hipMemsetAsync(P->arena, 0, (size_t)P->arena_floats * sizeof(float), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  for (OpDesc& op : P->ops) {
    if (op.kind != OP_CONV) continue;
    const auto it = h->tune_cache.find(conv_signature(op));
    if (it != h->tune_cache.end()) op.tile = it->second;   // (always there behind a measuring call; else the planner's default tile stays)
  }
  return FILM_OK;
}

}  // namespace film_internal

using namespace film_internal;

extern "C" {

// Autotune choices as text: a header line with the library version, then one "<conv shape signature>\t<tile id>" line per
// measured shape (this handle's own measurements + imported ones it has not needed yet).
int film_export_tune(film_t* h, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  std::ostringstream o;
  o << "# film_hip tune cache v1 " << film_version() << "\n";
  std::map<std::string, int> all = h->tune_import;
  for (const auto& kv : h->tune_cache) all[kv.first] = kv.second;
  for (const auto& kv : all) o << kv.first << '\t' << kv.second << '\n';
  return copy_out_string(h, o.str(), buf, cap, needed);
}

// Takes the text of film_export_tune.  A cache written by another library version is ignored (returns FILM_OK, imports
// nothing: tile ids are only meaningful within one build); entries are validated when a plan first needs them - a tile
// that is not a candidate of the op's kernel family is measured again.  Results never depend on the cache: every tile of
// a family produces the same bits.
int film_import_tune(film_t* h, const char* text) {
  if (!h || !text) return fail(h, FILM_ERR_INVALID, "NULL argument");
  std::istringstream in(text);
  std::string line;
  if (!std::getline(in, line)) return FILM_OK;
  const std::string want = std::string("# film_hip tune cache v1 ") + film_version();
  if (line != want) return FILM_OK;
  std::map<std::string, int> got;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    const size_t tab = line.rfind('\t');
    if (tab == std::string::npos || tab == 0 || tab + 1 >= line.size()) return fail(h, FILM_ERR_INVALID, "tune cache: malformed line '%s'", line.c_str());
    char* end = nullptr;
    const long tile = strtol(line.c_str() + tab + 1, &end, 10);
    if (*end != 0 || tile < 0 || tile > (1 << 20)) return fail(h, FILM_ERR_INVALID, "tune cache: malformed line '%s'", line.c_str());
    got[line.substr(0, tab)] = (int)tile;
  }
  for (const auto& kv : got) h->tune_import[kv.first] = kv.second;
  return FILM_OK;
}

}  // extern "C"
