// film_internal.h -- what the translation units of libfilm_hip.so share: the plan / op / layer / handle structures and the
// internal functions that cross file boundaries.  Nothing here is part of the C-ABI (include/film_hip.h).
//
//   film_engine.cpp   C-ABI entry points: handle lifetime, the option table, the JSON queries, tiling and chunking of film_forward /
//                     film_interpolate / film_interpolate_sequence, the host-buffer pipeline, taps, the debug entry points
//   film_stream.cpp   the frame streams (film_stream_*): the schedule of a push, where its frames live, the scene-cut rule, their JSON queries
//   film_exec.cpp     the executor: launch of one op, the two-lane issue, run_plan (eager, hipGraph capture / replay, profiling)
//   film_tune.cpp     the tile candidates of each kernel family, the autotuner, the tune cache as text
//   film_plans.cpp    the plan cache with its workspace arenas and eviction, the units-per-invocation limits
//   film_planner.cpp  the kernel decisions (family and split-K factor of a convolution: plain_conv_family / folded_conv_family / conv_ksplit),
//                     Planner: the graph of models/film_net/interpolator.py:89-207 as an op list over one workspace arena, one member
//                     function per stage; the two-lane dependency analysis; film_plan_json's text
//   film_layers.cpp   the layer table (weight names, shapes, channel permutations), the table of weight layouts and their packer
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/film_hip.h"
#include "film_kernels.h"

namespace film_internal {


extern thread_local std::string g_create_error;   // message of a failed film_create (film_engine.cpp)

enum OpKind { OP_CONV = 0, OP_FLOW_HEAD, OP_CONV_PW, OP_POOL, OP_FLOW_UP, OP_FLOW_ADD, OP_WARP, OP_PACK_FLOW, OP_KINDS };
extern const char* const kKindName[OP_KINDS];

struct Buffer {
  std::string name;
  int64_t off;  // floats from arena base
  int N, H, W, C;      // all 0 for scratch regions (reinterpreted per use)
  int64_t floats;      // extent
  // > 0: the buffer is stored as three pixel-major planes, [N][H][W][planar] x 2 then [N][H][W][C - 2 planar], instead of
  // [N][H][W][C] (the aligned pyramid levels: each plane is written contiguously by one warp launch; film_get_tap interleaves)
  int planar = 0;
  int64_t size() const { return floats; }
};

// A channel slice of (a batch range of) a workspace buffer, or of a scratch region.
struct View {
  int buf = -1;
  int64_t off = 0;  // floats from arena base to the first element of the view
  int stride = 0;   // floats per pixel
  int C = 0;
};

struct SegDesc {
  View v;
  int boff = 0, bmod = 0, up = 0;
};

// conv ops: the weight copies of the layer (ConvWeights; w_off is what conv_buf_kernel reads, = wf4_off when fold == 3), `family` the kernel
struct OpDesc : ConvWeights {
  int kind = 0;
  std::string tag;
  // conv
  SegDesc seg[FILM_MAX_SEG];
  int nseg = 0;
  int ksize = 1, leaky = 0, Cout = 0, Ctot = 0, tile = 0;
  ConvFamily family = FAM_BUF;        // conv: the kernel family (plain_conv_family / folded_conv_family, film_planner.cpp); tile carries its flag bits
  int64_t b_off = 0;
  int64_t w2_off = 0, b2_off = 0;     // flow_head: second 1x1 conv
  int ksplit = 1;                     // conv (conv_buf_kernel): split-K factor, partial sums at part_off (film_kernels.h)
  int64_t part_off = 0;
  int fold = 0, py = 0, px = 0;       // conv: sub-pixel phase of a folded upsample + 2x2 conv (H, W = low-res grid)
  int ftaps = 0; int tdy[4] = {0, 0, 0, 0}, tdx[4] = {0, 0, 0, 0};
  int64_t fold_woff[4] = {0, 0, 0, 0};  // fold == 2: weight offset of phase q relative to w_off
  int lane = 0;                       // graph replay: 0 = main stream, 1 = side stream (small / HBM-bound work)
  std::vector<int> xdeps;             // ops on the OTHER lane this op must wait for (from the buffer overlap analysis)
  bool signal = false;                // some op on the other lane waits for this one
  // generic views
  View in, in2, out;
  // warp: the fused sixteen miscellaneous channels of an aligned level (t = 0.5 stage): img_in = both images [2 NB][H][W][3],
  // pack_b / pack_f = backward / forward flow, img_out = [warp(img0) 3 | warp(img1) 3 | 0.5 bflow 2 | 0.5 fflow 2 | 0 x 6]
  View pack_b, pack_f;
  View img_in, img_out;
  View pw_out; int pw_cout = 0;   // conv: fused 1x1 convolution behind it (weights w2_off / b2_off) writes pw_out; `out` is not written then
  View in3, out2;   // warp: coarser flow to upsample / the upsampled flow it stores; flow heads: in2 = upsampled flow, out2 = v = out + in2
  int NB = 0, H = 0, W = 0;  // conv/warp: output dims; pool: input dims; flow_up: input dims
  float fscale = 1.f;
  int src_brot = 0, flow_brot = 0, misc_nb = 0;   // warp: one launch for both directions / images of a level (WarpParams)
  int64_t n = 0;
  double flops = 0;  // algorithmic FLOPs (reference channel counts)
  double bytes = 0;  // algorithmic bytes (read once + write once)
};

struct LayerPack : ConvWeights {   // (+ the offsets of its weight layouts)
  std::string name;
  int kh, kw, cin, cout;     // reference shape
  std::vector<int> perm;     // internal input channel -> reference input channel, -1 = zero row
  bool c3 = false;           // first layer: packed as [12 tap slots][4][Cout] (row = tap*4 + channel, rest zero)
  // layers run by the MFMA conv kernel (Cout % 32 == 0) are packed K-contiguous per output channel:
  // [Cout][kh*kw*ctot] with k = tap*ctot + channel; the 1x1 heads keep [ctot][Cout]
  bool kmajor() const { return !c3 && cout % 32 == 0; }
  int64_t b_off = 0;
  int64_t wf_off = -1;       // 2x2 layers behind a nearest upsample: the four sub-pixel phases, pre-summed weights (fill_wf, film_layers.cpp)
  bool has_halo() const { return kmajor() && kh == 3 && kw == 3; }
  bool has_fold() const { return kmajor() && kh == 2 && kw == 2; }
  bool has_fold4() const { return has_fold() && ctot() % 16 == 0 && cout % 32 == 0; }   // ... with the difference-form copy (conv_fold4_impl.h)
  // conv_wino2d_kernel against the best 1-D F(4,3) tile of the same run (tools/w2d_bench.hip, profiles/r04_w2d_vs_w43.log): 16-30 %
  // faster on EVERY 3x3 layer of the 1080p plan, K = 32 ... 2448 (round 3's kernel lost below K = 208: its four-round epilogue of dword
  // stores cost 26 000 cycles per workgroup) - every 3x3 layer whose channels come in sixteens and thirty-twos carries the copy
  bool has_w2d() const { return has_halo() && ctot() % 16 == 0 && cout % 32 == 0; }
  int ctot() const { return (int)perm.size(); }
  int64_t packed_rows() const { return c3 ? 48 : (int64_t)kh * kw * ctot(); }
};

struct HostTensor {
  std::vector<int64_t> dims;
  std::vector<float> data;
};

struct Plan {
  int B = 0, H = 0, W = 0;   // B = pair-tiles (frame pairs x tiles per pair)
  // 0: a pair plan (img0 = [x0 tiles | x1 tiles], 2B images); > 0: a sequence plan over B / tiles consecutive frame pairs of `tiles`
  // tiles each (img0 = B + tiles images, frame-major: image f * tiles + t; pair-tile p reads images p and p + tiles)
  int tiles = 0;
  // ---- stream plans only (film_stream_*) ----
  // A stream plan is the sequence plan of ONE pair of `tiles` tiles (B == tiles) over `slots` frame slots of `tiles` images each in the
  // per-image buffers (img*, feat*, extractor scratch): 2 for a plain stream - the two frames of a pair take turns - and T + 1 with option
  // "stream_times" = T: slots 0 and 1 take turns for the input frames, slot 1 + d holds the depth-d mid-frame that is fed back.
  // An ORIENTATION is (left, right, extract): image 0 of the pair is the frame in slot `left`, image 1 the one in slot `right`, and with
  // `extract` the image pyramid and feature ops of the right frame, NB = tiles, are ops [0, n_extract) - else the plan has none of them
  // (n_extract = 0: a plan of its own with its own lane analysis, never the tail of an extracting one).  right = -1: not a stream plan.
  // Ownership: the CACHE ENTRY (what get_plan returns; itself orientation (1, 0, extract)) owns the buffer layout, the id and the workspace,
  // and holds every other orientation in `orientations`, keyed by orientation_key.  An orientation owns its ops, events and graph and
  // borrows the rest (owns_arena = false): same bufs, same id, same arena pointer, gone with its entry.  plan_orientation (film_plans.cpp)
  // is the one way to an orientation: it finds it or builds it on first use.
  int slots = 0, left = -1, right = -1;
  bool extract = true;
  size_t n_extract = 0;
  bool owns_arena = true;
  std::map<int, std::unique_ptr<Plan>> orientations;
  static int orientation_key(int l, int r, bool e) { return (l * 16 + r) * 2 + (e ? 1 : 0); }
  bool holds(const Plan* q) const {   // q is this cache entry or one of its orientations
    return q == this || std::any_of(orientations.begin(), orientations.end(), [q](const auto& kv) { return kv.second.get() == q; });
  }
  // ----
  uint64_t id = 0;           // unique per handle and build: a stream tells a rebuilt plan (its carried features are gone) from the one it filled
  std::vector<Buffer> bufs;
  std::vector<OpDesc> ops;
  int64_t arena_floats = 0;
  float* arena = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  hipGraph_t graph = nullptr;
  std::vector<hipEvent_t> ev;
  std::vector<hipEvent_t> lane_ev;    // one per signalling op (index = op index), lazily created; + fork/join at the end
  uint64_t last_use = 0;
  int find(const std::string& n) const {
    for (size_t i = 0; i < bufs.size(); ++i)
      if (bufs[i].name == n) return (int)i;
    return -1;
  }
  float* at(const char* name) const { return arena + bufs[find(name)].off; }   // a buffer every plan has ("img0", "out") in the workspace
};

// The bits of option "fuse" (film_handle::opt_fuse; include/film_hip.h): small-launch fusion, identical arithmetic and bit-identical results
enum FuseBit {
  FUSE_FLOW_UP = 1,    // tf.image.resize(2 * v) of the flow estimator inside the warp kernels that consume it
  FUSE_FLOW_ADD = 2,   // v = residual + upsampled flow inside the flow-head kernels
  FUSE_MISC16 = 4,     // the warped images and the half flows of the t = 0.5 stage (the sixteen miscellaneous channels of an aligned level)
                       // inside the second feature warp of the level
  FUSE_POOL = 8,       // AveragePooling2D of the sub-extractor stages in the epilogue of the convolution in front of it
  FUSE_RGB_HEAD = 16,  // the RGB head (1x1 convolution, fusion.py:138-140) in the epilogue of the last decoder layer
};

}  // namespace film_internal

// film_stream_*: the one open stream of a handle.  The carried frame's pyramids live in the stream plan's workspace; `keep` is the
// stream's own copy of that frame (in its pixel type), from which they are rebuilt when the plan was evicted or dropped in between.
struct FilmStream {
  bool open = false;
  int H = 0, W = 0, align = 0, block_h = 0, block_w = 0, pix = 0;   // pix: a FILM_PIX_* layout plus, for 4:2:0, the FILM_YUV_* flags
  void* keep = nullptr;             // the last pushed frame: [H][W][3] float32 or bytes, or the H * W * 3 / 2 bytes of a 4:2:0 frame
  float* result = nullptr;          // the joined float32 mid-frame of a host or 8-bit push
  unsigned char* result8 = nullptr; // ... quantised (RGB bytes or a 4:2:0 frame, 8-bit or 10-bit), of a host push that is not float32
  int times = 1;                    // option "stream_times" when the stream was opened: a primed push writes 2^times - 1 frames; `result` (float32
                                    // streams) and `result8` hold that many frames, so that a host push downloads them behind one wait
  uint64_t mask = 1;                // film_stream_select: bit i - 1 = position i of a primed push is wanted; film_stream_open selects all
                                    // 2^times - 1, and neither film_stream_reset nor a scene cut changes it
  bool primed = false;              // `keep` holds a frame
  int slot = 0;                     // the half of the plan's frame buffers it was extracted into ...
  uint64_t plan_id = 0;             // ... of this plan (Plan::id) ...
  TileMapParams geo{};              // ... cut with this geometry (block_overlap_* may change between pushes)
  // option "scene_cut" (include/film_hip.h, "Scene cuts"); the two buffers are allocated by the first push that needs them
  uint32_t* hist_dev = nullptr;     // the 768 counters of the frame in `keep` ...
  uint32_t* hist_pin = nullptr;     // ... downloaded here (pinned host memory)
  uint32_t hist_prev[768] = {};     // the previous frame's histogram, on the host: a dropped plan does not touch it
  bool hist_valid = false;          // hist_prev is the histogram of the frame in `keep`
  int64_t cut_distance = -1;        // film_stream_cut_info: D of the last push (-1: no comparison made) ...
  int cut = 0;                      // ... and whether it was treated as a cut
  // option "dup_hi" (include/film_hip.h, "Duplicate frames"); the three buffers are allocated by the first push that needs them
  void* keep2 = nullptr;            // where such a push lands: compared with `keep`, then dropped or swapped with it
  uint64_t* diff_dev = nullptr;     // out[3][4] of the comparison ...
  uint64_t* diff_pin = nullptr;     // ... downloaded here (pinned host memory)
  int64_t dup_stats[12] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // film_stream_dup_info: out[3][4] of the last push (-1: no comparison made) ...
  int dup = 0;                      // ... and whether it was dropped as a duplicate
  // Tile groups (film_stream.cpp, "tile groups"): a frame whose tiles do not fit one invocation runs as `groups` runs of ONE stream plan of
  // group_tiles tiles, the last group with the tiles that are left.  Both are decided by film_stream_open and fixed for the stream's life.
  // groups == 1: the whole frame in one invocation, nothing below is used.
  int group_tiles = 0, groups = 1;
  float* carry = nullptr;           // groups > 1: per (group, frame slot) what a pair run reads of an extracted frame - the truth about the carried frame
  int64_t carry_floats = 0;         // ... its size (allocated again when "block_overlap_*" grows the padded tile)
};

struct film_handle {
  FilmStream fs;
  uint64_t plan_ids = 0;
  void* stage = nullptr;       // device staging of whole frames for film_interpolate(FILM_MEM_HOST)
  size_t stage_bytes = 0;
  void* metrics_buf = nullptr;  // film_image_metrics: partials + results (+ the images with FILM_MEM_HOST), grown on demand
  size_t metrics_bytes = 0;
  int device = -1;
  bool plan_only = true;
  film_config cfg{};
  hipStream_t stream = nullptr;
  std::string err;
  std::map<std::string, film_internal::HostTensor> host_w;
  std::vector<film_internal::LayerPack> layers;
  std::map<std::string, int> layer_idx;
  int64_t packed_floats = 0;          // floats of the PACKED PREFIX (groups [0, groups_packed)); group_end[3] = all layouts
  int64_t group_end[4] = {0, 0, 0, 0};  // end offset of weight layout group g (the groups: kLayouts, film_layers.cpp)
  int groups_packed = 0;
  std::vector<float> packed_host;
  float* packed_dev = nullptr;
  bool finalized = false;
  std::vector<std::unique_ptr<film_internal::Plan>> plans;
  film_internal::Plan* last_plan = nullptr;
  uint64_t tick = 0;
  // How a plan is executed (option "graph"): 2 (default) = its ops are launched directly on two lanes - lane 0 on the caller's stream,
  // lane 1 on the handle's side stream, ordered by the events of Planner::analyze_lanes; 1 = the same two lanes captured once into a
  // hipGraph and replayed; 0 = one stream, in plan order (the reference the tests compare the other two with: bit-identical).
  // Why the graph is not the default (round 5): the HIP runtime PyTorch 2.10+rocm7.0 bundles (7.0.51831) crashes in the FIRST
  // hipGraphLaunch of a freshly instantiated multi-branch graph when the process has created and destroyed enough streams before -
  // a null-ish dereference in the function that assigns the exec's parallel streams (reads past its own stream vector; backtrace and
  // disassembly: profiles/r05_hipgraph_first_launch_crash.md).  Reproduced by the GPU test-suite in file order (8 engines, 23 graphs
  // into the process); not reproducible in a short process.  A linear graph (lanes = 0) takes the runtime's single-stream path and
  // is safe but serial (+2 ms per 1080p step); direct launches cost ~170 runtime calls per forward on the host, asynchronously.
  int opt_graph = 2;
  int opt_profile = 0, opt_autotune = 1;
  int opt_max_batch = 0;  // 0: only the 4 GiB-per-buffer limit
  // Tiled path: pixels every tile takes from its neighbours on each side of an axis with more than one block; the tiles' results are
  // cross-faded over the shared pixels (tile_geometry in film_engine.cpp; blend_tiles_kernel).  0 (default): the reference's disjoint
  // patches.  -1: as much as the tile's align padding holds (the padded tile, and with it the plan, stays the same).
  int opt_block_overlap_h = 0, opt_block_overlap_w = 0;
  int opt_stream_times = 1;   // film_stream_open: T = 1 .. 6, a primed push of that stream writes the 2^T - 1 frames of the reference's recursion
  int opt_scene_cut = 0;      // film_stream_push: permille of the histogram distance from which a pair of frames is a scene cut (0: off)
  // film_stream_push: a pushed frame is a duplicate of the carried one iff, per plane, no 8 x 8 block SAD exceeds dup_hi and at most dup_frac
  // permille of the blocks exceed dup_lo (8-bit code units; x 4 on 10-bit layouts); dup_hi = -1: off, today's pushes
  int opt_dup_hi = -1, opt_dup_lo = 0, opt_dup_frac = 1000;
  int opt_host_overlap = 1;   // film_interpolate(FILM_MEM_HOST): 1 = the second frame's upload behind the first frame's first layers, the first half of the
                              // result downloaded behind the second half's last layer (film_engine.cpp, "host pipeline"); 0 = copies, then work, then copy
  hipEvent_t pipe_ev[2] = {nullptr, nullptr};   // its two events (second frame in place / first half stitched), lazily created
  int opt_splitk = 1;     // 1: split-K (ksplit partial sums + ordered reduction) for the deep layers of levels with <= 1024 pixels
  int opt_fuse = 31;      // FuseBit mask: flow_up fused into the flow-estimator warps, v = res + up into the flow heads, ... (same arithmetic, 12 launches fewer)
  int opt_planar = 1;     // 1: aligned-pyramid levels as three planes (feat0 | feat1 | misc16), each written contiguously by its warp
  int opt_fold2x2 = 1;    // != 0: nearest-upsample + 2x2 conv as four sub-pixel phase convolutions (9 taps per 4 outputs); 1: ... in the difference form
                          // on conv_fold4_kernel (4 multiplies per low-resolution pixel instead of 9)
  int opt_wino = 1;       // 0: never, 1: Winograd kernels (F(4,3) / F(2,3)) where measured faster (default), 2 / 3: F(2,3) / F(4,3) on every eligible 3x3 conv
  int opt_halo_all = 0;   // 1: halo / split kernels for every eligible 3x3 conv regardless of size (tests, tuning)
  int opt_tune_ms = 0;    // autotune: minimum kernel time spent per candidate (0: two launches)
  int opt_lanes = 1;      // >= 1: replay graphs use a second (side) stream for independent small / HBM-bound work; 2: and (large frames) for
                          // the coarse decoder levels, emitted right behind the aligned levels they read (measured SLOWER: 48.3-48.4 ms
                          // against 47.4-47.6 ms per 1080p step, profiles/r03_lanes_ab.log - two matrix-bound streams share the CUs
                          // worse than one; kept as a tested option, not the default)
  hipStream_t stream2 = nullptr;
  int opt_precision = 0;  // 0: fp32 MFMA everywhere (default); 1: bf16x6 exact-split MFMA for the large 3x3 convs; 2: bf16x3
  int opt_wino2d = 1;     // nested Winograd kernel: 0 never, 1 (default) the deep-K layers of the large levels, 2 every layer that has the copy (tests)
  int opt_w2d_min_px = 1536; // conv_wino2d_kernel runs the 3x3 layers of levels with at least this many pixels per image (planner rule;
                             // profiles/r04_w2d_min_px_ab.log: 8 or more 8x32 patches per image - 32x56 yes, 32x32 no)
  int opt_w2d_small_px = 256; // ... and of smaller levels down to this many pixels when the level fills >= 65 % of its 8x32 tiles (0: never)
  int opt_w2d_splitk = 1; // >= 1: split-K for the nested kernel's K >= 768 layers on levels of <= 4096 pixels, S = min(4, K / 384); 2..16: and a cap of that many
                          // K ranges on levels of <= 1024 pixels (planner rule; option "w2d_splitk" for A/B runs)
  int opt_w2d_shape = -1; // tests: >= 0 = every conv_wino2d_kernel op that can run this Wino2dTile shape does
  int opt_fold4_shape = -1; // tests: >= 0 = every conv_fold4_kernel op that can run this Fold4Tile shape does
  int opt_w43_shape = -1; // tests: >= 0 = every conv_wino43_kernel op that can run this Wino43Tile shape does (instead of the autotuned one)
  std::string profile_json;
  // option "profile": what run_plan has measured - of the last run, or (profile_append: a film_stream_push of several runs) of every run since the flag was set
  struct ProfileClass { int launches = 0; double ms = 0, flops = 0, bytes = 0; };
  bool profile_append = false;
  std::string profile_ops;
  std::map<std::string, ProfileClass> profile_classes;
  std::map<std::string, int> tune_cache;  // conv shape signature -> fastest tile
  std::map<std::string, int> tune_import; // choices of an earlier process (film_import_tune): taken, if still a candidate of
                                          // the op's kernel family, instead of timing the candidates again
};

extern "C" int film_ensure_groups_(film_t* h, int n);   // packs + uploads weight layout groups [groups_packed, n) on demand (internal)

namespace film_internal {

int fail(film_t* h, int code, const char* fmt, ...);    // stores the message on the handle (or for film_create), returns `code`

#define HIPCHK(h, expr)                                                                     \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(h, FILM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)


// ---- film_layers.cpp: architecture helpers (mirror frame-interpolation_amd/film_hip/weights.py) and the layer table
std::vector<int> feature_channels(const film_config& c);   // feature_extractor.py:186-193
int slot_offset(const film_config& c, int j);              // channel offset of sub-pyramid stage j in a feature level
std::vector<int> fusion_filters(const film_config& c);     // fusion.py:75-79
std::string predictor_prefix(const film_config& c, int level);   // pyramid_flow_estimator.py:109-123
int predictor_index(const film_config& c, int level);
int validate_config(film_t* h, const film_config& c);
void build_layers(film_t* h);
int layout_groups(int64_t ConvWeights::* copy);   // the weight layout groups [0, n) that must be packed before a kernel can read `copy`

// The per-op codes plan_json and the tune-cache signatures have always carried for a conv op's family: "c3", "halo", "split"
// (1 bf16x6, 2 bf16x3) and "wino" (1 F(2,3), 2 bf16x3 F(2,3), 3 F(4,3), 4 nested F(4,3) x F(2,3)).
struct FamilyCodes { int c3 = 0, halo = 0, split = 0, wino = 0; };
inline FamilyCodes family_codes(ConvFamily f) {
  FamilyCodes c;
  switch (f) {
    case FAM_C3: c.c3 = 1; break;
    case FAM_HALO: c.halo = 1; break;
    case FAM_SPLIT6: c.split = 1; break;
    case FAM_SPLIT3: case FAM_FOLDX3: c.split = 2; break;
    case FAM_WINO: c.wino = 1; break;
    case FAM_WINOX3: c.wino = 2; break;
    case FAM_W43: c.wino = 3; break;
    case FAM_W2D: c.wino = 4; break;
    default: break;
  }
  return c;
}

// ---- film_engine.cpp
int copy_out_string(film_t* h, const std::string& s, char* buf, int64_t cap, int64_t* needed);   // a text result of the C-ABI, or its size
int tile_geometry(film_t* h, int H, int W, int block_h, int block_w, int align, TileMapParams* tp);   // a frame cut into padded tiles, or a refusal
int check_pix(film_t* h, int pix, int H, int W);      // FILM_OK, or the refusal of a `pix` argument for H x W frames
int64_t frame_samples(int pix, int H, int W);         // samples of one H x W frame of pixel type `pix` ...
size_t frame_bytes(int pix, int H, int W);            // ... and its bytes
int need_device(film_t* h, const char* fn);           // the refusals the compute entry points share (`fn`: the entry point)
hipStream_t pick_stream(film_t* h, int mem_kind, void* stream);   // the stream a call with `stream` (NULL: the default of its mem_kind) works on
constexpr int kMaxStreamTimes = 6;                    // option "stream_times": 1 .. this
int balanced_chunk(int n, int maxc);                  // chunk size for n independent units, at most maxc per invocation
bool halve_on_nomem(int rc, int* chunk);              // the retry rule of the chunk loops

// ---- film_stream.cpp
void stream_free(film_t* h);   // the open stream's device buffers go back and it is closed (film_stream_close, film_destroy)

// ---- film_exec.cpp
hipError_t launch_op(const OpDesc& op, float* arena, const float* wts, hipStream_t s);
bool batch_splittable(const OpDesc& op, int nparts);
OpDesc batch_part(const OpDesc& op, int part, int nparts);
// Hooks of film_interpolate's host-buffer pipeline into the two-lane issue (see there): `head` = the leading main-lane convolutions that run per
// input frame (part 0 = the tiles of x0 - launched by the caller BEFORE the second frame's upload; issue_lanes launches part 1), `tail` = the
// last op (the decoder's last layer + RGB head) runs as two tile halves with `mid_tail` between them (stitch + download of the first half).
struct LanePipe {
  std::vector<size_t> head;
  bool tail = false;
  std::function<hipError_t()> mid_tail;
};
hipError_t issue_lanes(film_t* h, Plan* P, hipStream_t main, bool capturing, const LanePipe* lp = nullptr);
int run_plan(film_t* h, Plan* P, hipStream_t s, size_t n_ops = SIZE_MAX);   // n_ops < the plan's: its first n_ops ops only, on `s` alone

// ---- film_tune.cpp (the nine *_candidates of kConvFamily: film_kernels.h)
std::vector<int> conv_candidates(const OpDesc& op);
int autotune_plan(film_t* h, Plan* P, bool measure = true);   // !measure: only the choices made already (the workspace is not touched)

// ---- film_plans.cpp
int get_plan(film_t* h, int B, int H, int W, bool need_device, Plan** out, int tiles = 0, int slots = 0);   // slots >= 2: the stream plan, B == tiles
// orientation (left, right, extract) of the stream plan P0 (what get_plan returned): found, or built, tuned and cached with it on first use.
// (1, 0, extract) is P0 itself and (0, 1, extract) comes with it; nothing else looks for an orientation.
int plan_orientation(film_t* h, Plan* P0, int left, int right, bool extract, Plan** out);
void drop_plans(film_t* h);   // waits for the device, then frees every cached plan
int max_units(film_t* h, int H, int W, const char* what, const char* advice, int* units);

// ---- film_planner.cpp
// fills P->bufs / ops / arena_floats for (B, H, W) (tiles > 0: sequence plan; slots >= 2: orientation (left, right, extract) of the stream plan
// of that many frame slots, B == tiles)
int plan_build(film_t* h, Plan* P, int B, int H, int W, int tiles = 0, int slots = 0, int left = -1, int right = -1, bool extract = true);
int64_t limited_buffer_bytes(const Plan* P);                // largest buffer a kernel with whole-buffer 32-bit offsets reads
void op_views(const OpDesc& op, std::vector<const View*>& rd, std::vector<const View*>& wr);   // the views an op reads / writes
std::string plan_json(film_t* h, const Plan& P, bool orientation_keys = false);   // (a stream plan: "slot", or "slots", "left", "right")

}  // namespace film_internal
