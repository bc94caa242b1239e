// film_planner.cpp -- the planner: restates the *graph* of models/film_net/interpolator.py:89-207 as a static list of kernel
// launches over one workspace arena for a given (B,H,W):
//   image pyramids     util.py:23-45                -> pool ops on [2B,...,3] (both images in one batch)
//   feature extractor  feature_extractor.py:163-193 -> conv ops writing straight into the cascaded slots
//   flow estimator     pyramid_flow_estimator.py:125-163 -> both directions batched as 2B
//   flow synthesis     util.py:106-117              -> reuses the estimator's v (identical arithmetic)
//   warps + concat     interpolator.py:163-183      -> warp ops writing into the aligned pyramid
//   fusion             fusion.py:103-140            -> NN-upsample folded into the 2x2 conv's gather
// A sequence plan (tiles > 0) runs F - 1 consecutive pairs of F frames: the image pyramids and the extractor run once per
// frame (B + tiles images), every op that reaches the other image of a pair is emitted per direction with that image one
// pointer offset of `tiles` images away, and the flow estimator (2B) and the decoder (B) are the pair plan's.
// A stream plan is the sequence plan of ONE pair over `slots` frame slots of `tiles` images each (2: the two frames of a pair take turns
// between calls; T + 1 with option "stream_times" = T: one more slot per depth of mid-frames that are fed back).  An orientation (left,
// right, extract) reads the pair's earlier frame in slot `left` and its later one in slot `right`; with `extract` the per-image stages run
// on the `tiles` images of slot `right` only and come first in the op list (Plan::n_extract of them), else the plan has none of them.
// Every orientation lays out the same buffers at the same offsets and emits the same ops but for those image offsets.
// Top down: the kernel decisions (plain_conv_family / folded_conv_family / conv_ksplit: pure functions of a convolution's shape, its buffers'
// layout and the options - never of timing or the batch size), the Planner (a helper per op kind, a member per stage of the graph,
// Planner::build their sequence), the cross-lane dependencies of the two-stream replay (analyze_lanes), a plan as JSON (film_plan_json).
#include "film_internal.h"

namespace film_internal {

const char* const kKindName[OP_KINDS] = {"conv_mfma", "flow_head", "conv_pw", "pool", "flow_up", "flow_add", "warp", "pack_flow"};

// The views an op reads and the views it writes: what the lane analysis orders, and what tells a grouped stream which buffers a pair run only reads
void op_views(const OpDesc& op, std::vector<const View*>& rd, std::vector<const View*>& wr) {
  rd.clear(); wr.clear();
  if (op.kind == OP_CONV) { for (int i = 0; i < op.nseg; ++i) rd.push_back(&op.seg[i].v); }
  else { if (op.in.buf >= 0) rd.push_back(&op.in); if (op.in2.buf >= 0) rd.push_back(&op.in2); }
  if (op.in3.buf >= 0) rd.push_back(&op.in3);
  if (op.img_in.buf >= 0) rd.push_back(&op.img_in);
  if (op.pack_b.buf >= 0) { rd.push_back(&op.pack_b); rd.push_back(&op.pack_f); }
  if (op.out.buf >= 0 && op.pw_out.buf < 0) wr.push_back(&op.out);
  if (op.pw_out.buf >= 0) wr.push_back(&op.pw_out);
  if (op.out2.buf >= 0) wr.push_back(&op.out2);
  if (op.img_out.buf >= 0) wr.push_back(&op.img_out);
}

namespace {
// ---- kernel decisions ----------------------------------------------------------------------------------------------------------
// What the rules below decide from: the layer, the level and the layout of the buffers the convolution reads and writes (a property
// of the layer's buffers, so still a function of the layer only).  No batch size in here, on purpose.
struct ConvSite {
  const LayerPack* L;
  int H, W;               // the grid the kernel works on: the level - of a folded upsample + 2x2 conv, the LOW-resolution level it reads
  int ctot;               // input channels, all segments
  bool folded;            // nearest x2 + 2x2 conv as phase convolutions on the low-resolution input (Planner::conv)
  bool any_up;            // some segment is read through a nearest upsample (in the gather of conv_buf_kernel)
  bool out_16b;           // the output slice starts at 16-byte aligned pixels: offset and pixel pitch multiples of four floats
  bool segs_16b;          // ... and so does every input segment
  bool segs_c16;          // every input segment is a multiple of 16 channels
  bool halo_row_24bit;    // a halo row of every segment, W pixels x the pixel pitch, is below 2^24 bytes
  bool fold4_rows_32bit;  // eight output rows of conv_fold4_kernel (16 W pixels of the wider of pixel pitch and Cout) in 32-bit offsets
  int64_t px() const { return (int64_t)H * W; }   // pixels per image
};

ConvSite conv_site(const LayerPack& L, const std::vector<SegDesc>& segs, const View& out, int H, int W, bool folded) {
  ConvSite s{&L, H, W, 0, folded, false, out.off % 4 == 0 && out.stride % 4 == 0, true, true, true,
             (int64_t)16 * W * std::max(out.stride, L.cout) < (1ll << 31)};
  for (const SegDesc& g : segs) {
    s.ctot += g.v.C;
    s.any_up |= g.up != 0;
    s.segs_16b &= g.v.off % 4 == 0 && g.v.stride % 4 == 0;
    s.segs_c16 &= g.v.C % 16 == 0;
    s.halo_row_24bit &= (int64_t)W * g.v.stride * 4 < (1ll << 24);
  }
  return s;
}

// Kernel family of a plain convolution, by layer shape only (never by timing, and not by the batch size): the kernels sum K in a
// different order, so the choice must be a pure function of the layer for results to be reproducible across batch sizes and runs.
// Strongest rule first; a layer no rule takes runs on the general kernel (conv_buf_kernel).  `o`: the opt_* fields only.
ConvFamily plain_conv_family(const ConvSite& s, const film_t& o) {
  const LayerPack& L = *s.L;
  const int W = s.W, ctot = s.ctot;
  const int64_t px = s.px();
  // 1. Nested F(4,3)x x F(2,3)y (conv_wino2d_kernel, 1.5x fewer MFMAs than the 1-D form): EVERY 3x3 layer whose channels come in
  // sixteens (K = 32 ... 2448) on levels of at least opt_w2d_min_px pixels per image (default 1536: eight or more of its 8x32
  // patches per image; below that the 1-D kernel's split-K fills the chip better at batch 1).  A family of its own, a function of the
  // layer and the level size only.  A/B over the BASELINE configs: profiles/r04_w2d_min_px_ab.log.
  // conv_wino2d_kernel moves the halo patch by DMA in 16-channel pieces and stores four channels per lane: every input segment
  // a multiple of 16 channels at 16-byte aligned pixels, a 16-byte aligned output slice (true of every such layer of the
  // published net), and a halo row of a segment below 2^24 bytes - the DMA offsets are two 24-bit multiply-adds.
  const bool w2d_layout = ctot % 16 == 0 && s.out_16b && s.segs_c16 && s.segs_16b && s.halo_row_24bit;
  // ... and on SMALLER levels (>= opt_w2d_small_px = 256 pixels) whose shape fills at least 65 % of its 8-row x 32-pixel tiles:
  // 18x30 (a 1080p tile's level 5: 70 %), 32x32 (a 256x256 pair: 100 %), 16x28 (a 448x256 pair: 87 %) yes, 16x16 (50 %) and 9x15 (26 %)
  // no - its split-K fills the chip where the tile count does not.  A/B of the threshold over three configs:
  // profiles/r06_w2d_small_levels_ab.log (256x256 2.43 -> 2.35 ms, eight 448x256 pairs 15.7 -> 15.1, 1080p -0.1 ms).
  const int64_t w2d_tile_px = (int64_t)((s.H + 7) / 8) * 8 * ((W + 31) / 32) * 32;
  const bool w2d_level = px >= o.opt_w2d_min_px || (o.opt_w2d_small_px > 0 && px >= o.opt_w2d_small_px && px * 100 >= 65 * w2d_tile_px);
  if (L.w2d_off >= 0 && w2d_layout && !s.any_up && o.opt_precision == 0 &&
      (o.opt_wino2d == 2 || (o.opt_wino2d == 1 && o.opt_wino == 1 && w2d_level)))
    return FAM_W2D;
  // 2. Precision mode bf16x6: every 3x3 conv that is large enough to be matrix-pipe bound (conv_halo_split_kernel; bf16x3: same kernel,
  // two planes and three products - but see 3.)  (opt_halo_all: tuning / test knob, every eligible 3x3 conv, whatever its size)
  const bool split = o.opt_precision != 0 && L.has_halo() && !s.any_up && (px >= 2048 || o.opt_halo_all);
  if (split && o.opt_precision == 1) return FAM_SPLIT6;
  // 3. Winograd along x: where the 1.5x MFMA saving of F(2,3) survives its LDS / occupancy cost - wide N, large M.
  // F(4,3) needs the level width to fill its 64-pixel patches (at most 15 % of the last patch of a row empty)
  // (levels below 2048 pixels: its Q8 tiles take 32-pixel patches - the 32x32 level of a 256x256 frame)
  const bool w43_width = L.w43_off >= 0 && (o.opt_wino == 3 || 64 * ((W + 63) / 64) * 100 <= 115 * W ||
                                            (px < 2048 && 32 * ((W + 31) / 32) * 100 <= 115 * W));
  // deep K on a small level (the 36x60 level of a 1080p tile, K = 1920; down to 1024 pixels - the K = 1920 / 2448 layers of
  // the 32x32 level of a 256x256 frame ran 180-230 us each on the direct kernel, 0.4 of that frame's 2.8 ms): only with F(4,3) AND
  // its split-K, which cuts the few long workgroups of such a layer into enough pieces to fill the chip
  const bool deep_small = L.cout % 128 == 0 && px >= 1024 && px < 8192 && ctot > 1024 && w43_width && o.opt_splitk &&
                          o.opt_wino == 1 && o.opt_precision == 0;
  if (L.ww_off >= 0 && !s.any_up && o.opt_wino != 0 &&
      ((L.cout % 128 == 0 && (px >= 8192 || (px >= 2048 && ctot <= 1024))) || (L.cout % 64 == 0 && px >= 30000) ||
       px >= 100000 || o.opt_wino >= 2 || deep_small)) {
    if (o.opt_precision == 2 && (split || o.opt_wino >= 2)) {
      // bf16x3: the same layers run the Winograd form of the split kernel, conv_winox3_kernel.  It wins with the 2 x 2 wave block of
      // its 128-channel tile (0.88-0.94x the time of conv_halo_split_kernel<..,3> per layer, 427 vs 367 TFLOP/s at K = 22 032) and
      // loses with the 64-channel tiles (1.08-1.30x: twice the A staging per MFMA) - per-op profiles of the two plans and
      // conv_bench.hip (it left the tree in round 5; profiles/r01_conv_bench_x3.log) agree.  The 64-channel layers go on to rule 4.
      if (L.cout % 128 == 0 || o.opt_wino >= 2) return FAM_WINOX3;
    } else {
      // fp32: F(4,3) along x (conv_wino43_kernel, 2x fewer MFMAs than direct where F(2,3) has 1.5x) on the levels whose width
      // fills its 64-pixel patches (the Q16 tiles; at most 15 % of the last patch of a row empty: 960 ... 60, 448, 256 ...), else
      // F(2,3) (conv_wino_kernel).  "winograd" = 2 / 3 force F(2,3) / F(4,3) onto every eligible layer (tests).
      return o.opt_wino != 2 && w43_width ? FAM_W43 : FAM_WINO;
    }
  }
  // 4. Precision mode bf16x3 on the split kernel
  if (split) return FAM_SPLIT3;
  // 5. Halo staging pays where K is deep (traffic bound) or N is too narrow to amortise the per-tap A gather; measured in
  // conv_bench.hip (it left the tree in round 5; profiles/HISTORY.md 4.1).
  if (L.has_halo() && !s.any_up && (o.opt_halo_all || (px >= 8192 && (ctot >= 768 || (ctot >= 512 && px >= 100000) || L.cout == 32))))
    return FAM_HALO;
  return FAM_BUF;
}

// Kernel family of a folded upsample + 2x2 conv (s.H, s.W: the low-resolution level).
ConvFamily folded_conv_family(const ConvSite& s, const film_t& o) {
  const LayerPack& L = *s.L;
  // precision mode bf16x3: one halo-staged patch, nine (tap, phase) steps (conv_foldx3_kernel)
  if (o.opt_precision == 2 && L.wfx_off >= 0 && L.cout % 64 == 0 && (s.px() >= 2048 || o.opt_halo_all)) return FAM_FOLDX3;
  // the difference form (conv_fold4_impl.h): four GEMMs over K on I, Dx, Dy, Dxy - 4 multiplies per low-resolution pixel, not 9.
  // Its own summation family, chosen by the layer alone (every folded layer whose channels come in sixteens).  conv_fold4_launch's
  // layout checks: 16-byte aligned input and output pixels, 32-channel blocks, eight output rows in 32-bit offsets.
  if (o.opt_fold2x2 == 1 && o.opt_precision == 0 && L.wf4_off >= 0 && s.segs_16b && s.out_16b && L.cout % 32 == 0 && s.fold4_rows_32bit)
    return FAM_FOLD4;
  return FAM_BUF;   // four phase convolutions on the general kernel
}

// Split-K factor (1: none) of a convolution that runs on family `fam`: the K loop is cut into that many ranges, the partial sums are
// added in split order by conv_splitk_reduce_kernel (no atomics).  From the level size and the layer only - never the batch - so
// results stay independent of the batch size.
int conv_ksplit(ConvFamily fam, const ConvSite& s, const film_t& o) {
  const LayerPack& L = *s.L;
  const int ctot = s.ctot;
  const int64_t px = s.px();
  if (!o.opt_splitk || L.cout % 4 != 0) return 1;
  switch (fam) {
    case FAM_BUF: {
      // The deep layers of the coarse levels: the whole K loop (up to 1377 steps) of such a layer otherwise runs
      // on a handful of workgroups and IS the latency of the level (0.39 ms per flow-predictor conv_0 at 16 pixels).
      if (s.folded || !L.kmajor() || px > 4096) return 1;   // (the four-phase launch of a folded layer has no split form)
      const int nsteps = L.kh * L.kw * ctot / 16;
      // shallow layers: the extra launch costs more than it saves
      int S = nsteps < 128 ? 1 : px <= 64 ? 16 : px <= 256 ? 8 : px <= 1024 ? 4 : nsteps >= 256 ? 2 : 1;
      while (S > 1 && nsteps / S < 32) S >>= 1;
      return S;
    }
    case FAM_W43:
      // The F(4,3) kernel on levels whose workgroup count does not fill the 512 workgroup slots of the chip
      // evenly: a 72x120 level with 512 output channels is 1152 workgroups = 2.25 rounds, the last one on a quarter of
      // the CUs for the full duration of a deep K loop.  Two K ranges double the workgroup count at half the length.
      // 72x120 level, measured (profiles/r02_per_op_profile.json vs the run before): -10 % on the K = 2448 / 1920 layers,
      // +7..10 % on its K <= 512 layers (reduce kernel + twice the prologues / epilogues) -> deep K only
      // small levels (<= 4096 pixels per image: the 36x60 level of a 1080p tile, the 64x64 level of a 256x256 frame) have
      // 9-16 patches per image and channel block: K ranges of >= 128 channels, up to 8 of them (A/B on the GPU: 36x60 level
      // 2.90 -> 2.31 ms per 1080p step incl. its K = 1920 layer moving here from conv_buf_kernel; 64x64 level of a 256x256
      // pair 1.05 -> 0.86 ms; K < 512 left alone - the split would also undo the fused pooling of those layers)
      if (px <= 4096 && ctot >= 512) return std::min(8, ctot / 128);
      if (px <= 16384 && ctot >= 1024) return 2;
      return 1;
    case FAM_W2D: {
      // The nested kernel, on the SMALL levels only (<= 4096 pixels per image: the 36x60 level of a 1080p tile - 640
      // workgroups of its K = 1920 layer on 512 slots - and the 64x64 level of a 256x256 pair, 64-128 workgroups): K >= 768, up to four
      // K ranges.  Measured (profiles/r05_w2d_splitk.log): K = 1920 @ 8x36x60 0.653 -> 0.531 ms (0.61 -> 0.54 in the forward), K = 1168 @
      // 1x64x64 0.152 -> 0.084 ms, 256x256 pair 2.91 -> 2.82 ms.  NOT on the 72x120 level: its K = 1920 / 2448 layers are 2304 workgroups
      // = 4.5 rounds of the 512 slots and two K ranges gain 2-4 % stand-alone, but nothing in the forward (1.84 -> 1.89, 2.48 -> 2.49-2.53
      // ms per layer with the weights streaming from HBM and the partial sums written and read back: 141 MB for the K = 2448 layer).
      // No layer with a fused pool / 1x1 head is that deep.
      if (!o.opt_w2d_splitk) return 1;
      int S = 1;
      if (px <= 4096 && ctot >= 768) S = std::min(4, ctot / 384);
      if (o.opt_w2d_splitk > 1 && px <= 1024 && ctot >= 384) S = std::min(o.opt_w2d_splitk, ctot / 192);   // A/B knob: a higher cap on tiny levels
      return S;
    }
    case FAM_FOLD4:
      // Like the nested kernel's, for deep K on a TINY level: the decoder's coarsest layer of a 256x256 pair (K = 1936 on
      // 16x16 low-resolution pixels = 4 pixel tiles x 16 channel blocks: 64 workgroups of 242 chunks) 0.139 -> 0.048 ms with four K
      // ranges; on the 36x60 level of a 1080p tile (1152 workgroups) every split LOSES (0.589 -> 0.61-0.64 ms), eight 448x256 pairs
      // (16x28) lose 10 % (tools/fold4_bench, profiles/r06_fold4_bench.log).
      return px <= 1024 && ctot >= 768 ? 4 : 1;
    default:
      return 1;
  }
}

// ---- Planner ---------------------------------------------------------------------------------------------------------------------
struct Planner {
  film_t* h;
  Plan* P;
  int64_t cursor = 0;
  bool bad = false;
  std::string bad_msg;
  void refuse(const std::string& msg) { bad = true; bad_msg = msg; }   // build() fails with the LAST message

  // what the stages of build() share: the frame geometry ...
  int B = 0, T = 0, H0 = 0, W0 = 0;   // pair-tiles, tiles per frame of a sequence plan (0: pair plan), frame size
  int NL = 0, FL = 0;                 // pyramid levels, fusion (decoder) levels
  int N2 = 0, NI = 0;                 // 2B; images in the per-image buffers (image pyramids, features, extractor scratch)
  int i0 = 0, i1 = 0;                 // image 0 / image 1 of pair-tile b is image b + i0 / b + i1 of those buffers
  int NE = 0, e0 = 0;                 // the per-image stages run on images [e0, e0 + NE): all NI of them, or (stream plan) the pushed frame's
  bool seq = false;
  std::vector<int> fc, ff;            // feature channels / decoder filters per level
  int HL(int l) const { return H0 >> l; }
  int WL(int l) const { return W0 >> l; }
  // ... the buffer ids ...
  std::vector<int> img, feat, fx_a, fx_p, res, v, vup, warped, aligned, fu_u, fu_a, fu_b;
  int fp[3] = {-1, -1, -1}, out_buf = -1;
  View net;                           // ... and the decoder's running activation

  int push(const Buffer& b) {
    cursor += (b.floats + 63) & ~int64_t(63);  // 256-byte alignment
    P->bufs.push_back(b);
    return (int)P->bufs.size() - 1;
  }
  int add_buffer(const std::string& name, int N, int H, int W, int C) { return push(Buffer{name, cursor, N, H, W, C, (int64_t)N * H * W * C}); }
  int add_scratch(const std::string& name, int64_t floats) { return push(Buffer{name, cursor, 0, 0, 0, 0, std::max<int64_t>(floats, 64)}); }
  // view of channels [coff, coff+C) of batches [batch0, ...) of a buffer
  View view(int buf, int batch0, int coff, int C) const {
    const Buffer& b = P->bufs[buf];
    return View{buf, b.off + (int64_t)batch0 * b.H * b.W * b.C + coff, b.C, C};
  }
  // Part 0 / 1 / 2 of an aligned-pyramid level = warp(features of image 0) / warp(features of image 1) / the sixteen
  // miscellaneous channels.  Interleaved buffer: channel slices of [N][H][W][2C + 16]; planar buffer: three pixel-major planes.
  View aligned_part(int buf, int part, int C) const {
    const Buffer& b = P->bufs[buf];
    const int Cp = part < 2 ? C : 16;
    return b.planar ? View{buf, b.off + (int64_t)part * b.N * b.H * b.W * C, Cp, Cp} : view(buf, 0, part * C, Cp);
  }
  static View sub(View v, int coff, int C) { v.off += coff; v.C = C; return v; }
  // scratch view: reinterpret the start of a scratch buffer as [*][*][*][C]
  View scratch(int buf, int C) const { return View{buf, P->bufs[buf].off, C, C}; }
  // ... of the extractor subtree at level i: the images the per-image stages run on start e0 images of the subtree's FIRST stage (its
  // largest use: `per_image` floats each) into the region, whatever the stage - half way with the second frame of a stream plan
  View fx_scratch(int buf, int C, int64_t per_image) const { View v = scratch(buf, C); v.off += e0 * per_image; return v; }
  static SegDesc seg(View v, int up = 0) { SegDesc s; s.v = v; s.up = up; return s; }
  const LayerPack& layer(const std::string& name) const { return h->layers[h->layer_idx.at(name)]; }
  void to_lane(size_t first_op, int lane) { for (size_t q = first_op; q < P->ops.size(); ++q) P->ops[q].lane = lane; }

  // the weight layout group a kernel family reads must be packed (and on the device) before the plan can run
  void need_groups(int n) {
    if (!h->finalized || n <= h->groups_packed) return;
    if (film_ensure_groups_(h, n) != FILM_OK) refuse(h->err);
  }

  // The op runs on family `fam` - on conv_buf_kernel where this build of the library lacks it (the default library: film_set_option
  // refuses the options that ask for the opt-in families; a layer the nested / F(4,3) kernels cannot take runs on the general kernel).
  // M: the output pixels the default conv_buf_kernel tile is chosen for.
  void set_family(OpDesc& op, ConvFamily fam, int64_t M) {
    if (!conv_family_built(fam)) fam = FAM_BUF;
    op.family = fam;
    need_groups(layout_groups(kConvFamily[fam].weights));
    op.tile = conv_default_tile(fam, op.Cout, M);
  }

  // The ONE place that gives an op its split-K partial sums: S (> 1) x the op's output pixels x Cout floats.  A folded op (fold != 0)
  // runs on the low-resolution grid H x W and writes the 2H x 2W one.
  void split_k(OpDesc& op, int S) {
    op.ksplit = S;
    const int64_t out_px = (int64_t)op.NB * op.H * op.W * (op.fold ? 4 : 1);
    op.part_off = P->bufs[add_scratch("splitk:" + op.tag, S * out_px * op.Cout)].off;
  }

  // A convolution of the MFMA kernels: `segs` (channel slices, concatenated) -> `out`, H x W output pixels per image.
  void conv(const std::string& tag, const std::string& name, std::vector<SegDesc> segs, View out, int NB, int H, int W, bool leaky) {
    const LayerPack& L = layer(name);
    // nearest x2 + 2x2 'same' conv == four phase convolutions on the low-resolution input: kernel tap (dy, dx) of
    // output (2y+py, 2x+px) reads input ((2y+py+dy)>>1, (2x+px+dx)>>1) = (y + (py&dy), x + (px&dx)), so phase
    // (0,0) has ONE distinct input pixel, (0,1) and (1,0) two, (1,1) four: 9 taps per 4 outputs instead of 16.
    // The weights of taps that read the same pixel are summed at film_finalize (exact regrouping of the sum).
    // One launch runs the four phases (blockIdx.z): 4x the blocks of a phase launch, better tails.
    const bool folded = h->opt_fold2x2 != 0 && L.wf_off >= 0 && segs.size() == 1 && segs[0].up && !(H & 1) && !(W & 1);
    const ConvSite s = conv_site(L, segs, out, folded ? H / 2 : H, folded ? W / 2 : W, folded);
    OpDesc op;
    op.kind = OP_CONV;
    op.tag = tag + ":" + name + (folded ? ":phases" : "");
    op.nseg = (int)segs.size();
    for (int i = 0; i < op.nseg && i < FILM_MAX_SEG; ++i) op.seg[i] = segs[i];
    op.ksize = L.kh; op.leaky = leaky; op.Cout = L.cout; op.Ctot = s.ctot;
    op.out = out; op.NB = NB; op.H = s.H; op.W = s.W;
    static_cast<ConvWeights&>(op) = L;
    op.b_off = L.b_off;
    if (s.ctot != L.ctot() || out.C != L.cout || op.nseg > FILM_MAX_SEG || !L.kmajor()) refuse("planner: channel mismatch at " + tag + ":" + name);
    // every MFMA convolution stores dwordx4 (four channels of a pixel per lane): the destination slice must start on a multiple of
    // four floats of a pixel whose pitch is one.  film_create only accepts configurations (filters % 32 == 0, flow filters 32 or
    // % 64) for which every slice does; a layout that breaks this must fail HERE with a message, not as hipErrorInvalidValue at
    // launch time
    if (!folded && (!s.out_16b || L.cout % 32 != 0))
      refuse("planner: " + op.tag + " writes " + std::to_string(L.cout) + " channels at float offset " + std::to_string(out.off) + " of a " +
                std::to_string(out.stride) + "-float pixel: the convolution kernels need Cout % 32 == 0 and 16-byte aligned output slices");
    set_family(op, folded ? folded_conv_family(s, *h) : plain_conv_family(s, *h), (int64_t)NB * s.H * s.W * (folded ? 2 : 1));
    if (folded) {   // fold 3: the difference form, one weight copy; fold 2: the four phases, phase q's weights fold_woff[q] behind w_off
      op.seg[0].up = 0;
      op.fold = op.family == FAM_FOLD4 ? 3 : 2;
      op.w_off = op.fold == 3 ? L.wf4_off : L.wf_off;
      int64_t rel = 0;
      for (int q = 0; q < 4 && op.fold == 2; ++q) { op.fold_woff[q] = rel; rel += (int64_t)((q >> 1) + 1) * ((q & 1) + 1) * s.ctot * L.cout; }
    }
    const int S = conv_ksplit(op.family, s, *h);   // (of the family the op really runs on)
    if (S > 1) split_k(op, S);
    const double out_px = (double)NB * H * W;
    op.flops = 2.0 * out_px * L.cout * L.kh * L.kw * L.cin;   // algorithmic FLOPs of the reference op
    op.bytes = 4.0 * out_px * ((folded ? L.cin / 4.0 : L.cin) + L.cout);   // (folded: the low-resolution input is what is read)
    P->ops.push_back(op);
  }
  // the first layer of a sub-extractor: 3 image channels -> out.C, its own kernel (conv_c3_kernel)
  void conv_c3(const std::string& tag, const std::string& name, View in, View out, int NB, int H, int W) {
    const LayerPack& L = layer(name);
    OpDesc op;
    op.kind = OP_CONV; op.family = FAM_C3; op.tag = tag + ":" + name;
    op.nseg = 1; op.seg[0].v = in;
    op.ksize = 3; op.leaky = 1; op.Cout = out.C; op.Ctot = 3;
    op.w_off = L.w_off; op.b_off = L.b_off;
    op.out = out; op.NB = NB; op.H = H; op.W = W;
    op.tile = conv_default_tile(FAM_C3, out.C, 0);
    op.flops = 2.0 * NB * H * W * out.C * 27; op.bytes = 4.0 * NB * H * W * (3 + out.C);
    P->ops.push_back(op);
  }
  void conv_pw(const std::string& tag, const std::string& name, View in, View out, int64_t M, bool leaky) {
    const LayerPack& L = layer(name);
    OpDesc op;
    op.kind = OP_CONV_PW; op.tag = tag + ":" + name;
    op.in = in; op.out = out; op.n = M; op.leaky = leaky; op.Cout = L.cout; op.Ctot = L.cin;
    op.w_off = L.w_off; op.b_off = L.b_off;
    op.flops = 2.0 * M * L.cout * L.cin; op.bytes = 4.0 * M * (L.cin + L.cout);
    P->ops.push_back(op);
  }
  void pool(const std::string& tag, View in, View out, int NB, int H, int W) {
    OpDesc op;
    op.kind = OP_POOL; op.tag = tag; op.in = in; op.out = out; op.NB = NB; op.H = H; op.W = W;
    op.bytes = 4.0 * NB * H * W * in.C * 1.25;
    P->ops.push_back(op);
  }
  void warp(const std::string& tag, View src, View flow, View dst, int NB, int H, int W, float fscale,
            bool count_flow = true) {
    OpDesc op;
    op.kind = OP_WARP; op.tag = tag; op.in = src; op.in2 = flow; op.out = dst;
    op.NB = NB; op.H = H; op.W = W; op.fscale = fscale;
    // read source once + flow, write once.  The image part of a [image|features] warp is
    // a second launch here; its re-read of the flow is not algorithmic traffic.
    op.bytes = 4.0 * NB * H * W * (2.0 * src.C + (count_flow ? 2 : 0));
    P->ops.push_back(op);
  }

  // ---- the stages of the graph, in the order build() emits them ------------------------------------------------------------
  void add_buffers() {
    const film_config& c = h->cfg;
    for (int l = 0; l < NL; ++l) img.push_back(add_buffer("img" + std::to_string(l), NI, HL(l), WL(l), 3));
    for (int l = 0; l < NL; ++l) feat.push_back(add_buffer("feat" + std::to_string(l), NI, HL(l), WL(l), fc[l]));
    // feature-extractor scratch: stage-j conv_2j output and pooled input, sized for the largest use - stage 0's: every further
    // stage has a quarter of the pixels and twice the channels (H and W are multiples of 2^(levels - 1): the halvings are exact).
    // one scratch pair per pyramid level's subtree: the subtrees are independent chains (two of them run beside the
    // rest on the side stream of the replay graph) and 288 GB of HBM makes sharing pointless
    for (int i = 0; i < NL; ++i) {
      const bool pooled = std::min(NL - i, c.sub_levels) > 1;   // a one-stage subtree pools nothing
      fx_a.push_back(add_scratch("scratch_fx_a" + std::to_string(i), (int64_t)NI * HL(i) * WL(i) * c.filters));
      fx_p.push_back(add_scratch("scratch_fx_p" + std::to_string(i), pooled ? (int64_t)NI * HL(i + 1) * WL(i + 1) * c.filters : 0));
    }
    int64_t fp_sz = 0;
    for (int l = 0; l < NL; ++l) fp_sz = std::max<int64_t>(fp_sz, (int64_t)N2 * HL(l) * WL(l) * c.flow_filters[predictor_index(c, l)]);
    for (int k = 0; k < 3; ++k) fp[k] = add_scratch("scratch_fp_" + std::to_string(k), fp_sz);
    for (int l = 0; l < NL; ++l) res.push_back(add_buffer("res" + std::to_string(l), N2, HL(l), WL(l), 2));
    for (int l = 0; l < NL - 1; ++l) {
      vup.push_back(add_buffer("vup" + std::to_string(l), N2, HL(l), WL(l), 2));
      v.push_back(add_buffer("v" + std::to_string(l), N2, HL(l), WL(l), 2));
      warped.push_back(add_buffer("warped" + std::to_string(l), N2, HL(l), WL(l), fc[l]));
    }
    v.push_back(res[NL - 1]);  // coarsest: the DC term is the flow itself (pyramid_flow_estimator.py:149-150)
    // Planar aligned levels: the two feature warps and the miscellaneous channels of a level each write ONE contiguous plane
    // (256 ... 3840 contiguous bytes per pixel and launch) instead of 256-byte pieces at the 576-byte ... 7.7-KB pixel pitch of an
    // interleaved [feat0 | feat1 | misc16] pixel - the t = 0.5 warps then run like the flow-estimator warps of the same size
    // (0.28 -> 0.20 ms on the 576x960x64 level) - and the decoder reads the planes as three input segments in the same channel
    // order (same weights, same sums).  The coarsest fusion level stays interleaved: its only reader is the folded 2x2 layer,
    // which takes one segment.
    for (int l = 0; l < FL; ++l) {
      aligned.push_back(add_buffer("aligned" + std::to_string(l), B, HL(l), WL(l), 2 * fc[l] + 16));
      if (h->opt_planar && l < FL - 1 && fc[l] % 16 == 0) P->bufs[aligned[l]].planar = fc[l];
    }
    for (int i = 0; i < FL - 1; ++i) {
      fu_u.push_back(add_buffer("fusion_up" + std::to_string(i), B, HL(i), WL(i), ff[i]));
      fu_a.push_back(add_buffer("fusion_a" + std::to_string(i), B, HL(i), WL(i), ff[i]));
      fu_b.push_back(add_buffer("fusion_b" + std::to_string(i), B, HL(i), WL(i), ff[i]));
    }
    out_buf = add_buffer("out", B, H0, W0, 3);
  }

  // image pyramids (util.py:23-45), both images as one batch of 2B (sequence: every frame once)
  void emit_image_pyramids() {
    for (int l = 0; l + 1 < NL; ++l) {
      pool("image_pyramid_l" + std::to_string(l + 1), view(img[l], e0, 0, 3), view(img[l + 1], e0, 0, 3), NE, HL(l), WL(l));
      // on the side stream: the level-0 subtree (main stream) reads img[0] only and starts at once; six 6-us launches less in front of it
      // (256x256: 2.31 -> 2.28 ms per step, 1080p: -0.1 ms; profiles/r06_pool_lane_ab.log)
      P->ops.back().lane = 1;
    }
  }

  // cascaded feature extractor (feature_extractor.py:163-193): the subtree that starts at pyramid level i
  void emit_extractor(int i) {
    const film_config& c = h->cfg;
    const int n = std::min(NL - i, c.sub_levels);
    const size_t first_op = P->ops.size();
    const int64_t a_img = (int64_t)HL(i) * WL(i) * c.filters, p_img = (int64_t)HL(i + 1) * WL(i + 1) * c.filters;   // scratch floats per image
    for (int j = 0; j < n; ++j) {
      const int lv = i + j, k = c.filters << j;
      const std::string tg = "feat_s" + std::to_string(i) + "_" + std::to_string(j);
      const std::string w0 = "feat_net/sub_extractor/cfeat_conv_" + std::to_string(2 * j);
      const std::string w1 = "feat_net/sub_extractor/cfeat_conv_" + std::to_string(2 * j + 1);
      View tmp = fx_scratch(fx_a[i], k, a_img);
      if (j == 0) conv_c3(tg, w0, view(img[i], e0, 0, 3), tmp, NE, HL(lv), WL(lv));
      else conv(tg, w0, {seg(fx_scratch(fx_p[i], k >> 1, p_img))}, tmp, NE, HL(lv), WL(lv), true);
      View dst = view(feat[lv], e0, slot_offset(c, j), k);
      conv(tg, w1, {seg(tmp)}, dst, NE, HL(lv), WL(lv), true);
      if (j == n - 1) continue;
      OpDesc& cv = P->ops.back();
      if ((h->opt_fuse & FUSE_POOL) && cv.kind == OP_CONV && kConvFamily[cv.family].fused_shape >= 0 && cv.ksplit <= 1 && !(HL(lv) & 1) && !(WL(lv) & 1)) {
        // AveragePooling2D in the epilogue of the Winograd kernels (a lane / thread holds both rows of a 2x2 block)
        cv.tag += "+pool";
        cv.out2 = fx_scratch(fx_p[i], k, p_img);
      } else
        pool(tg + ":pool", dst, fx_scratch(fx_p[i], k, p_img), NE, HL(lv), WL(lv));
    }
    // every subtree but the level-0 one (75 % of the extractor's FLOPs) goes to the side stream: they and the coarse
    // flow levels that need only them are small, latency-bound launches that hide under the level-0 subtree
    // Small frames are latency bound: the flow chain l6 -> l0 can only start when the coarse subtrees (3..6) are done,
    // so those go first on the side stream while the main stream works through subtrees 0, 1, 2 (256x256: level-3 flow
    // starts after ~1.0 ms instead of ~1.5 ms).  Large frames keep subtrees 1.. on the side stream (tail filling).
    const int side_from = (int64_t)H0 * W0 <= 512 * 512 ? 3 : 1;
    if (i >= side_from) to_lane(first_op, 1);
  }

  // bidirectional coarse-to-fine flow (pyramid_flow_estimator.py:125-163), level l.
  // batch n = d*B + b: d = 0 forward (a = image 0, b = image 1), d = 1 backward.
  void emit_flow(int l) {
    const film_config& c = h->cfg;
    const size_t first_op = P->ops.size();
    const std::string tg = "flow_l" + std::to_string(l);
    const int pi = predictor_index(c, l);
    const int nf = c.flow_filters[pi], nconv = c.flow_convs[pi];
    const std::string prefix = predictor_prefix(c, l);
    const int Hl = HL(l), Wl = WL(l);
    const bool coarsest = l == NL - 1;
    if (!coarsest) {
      // the other image's features warped by the upsampled flow of level l + 1 (into warped[l]; the flow into vup[l])
      // tf.image.resize(2 * v) inside the warps that consume it (FUSE_FLOW_UP) pays on the small, launch-bound levels; on the
      // large ones every (pixel, channel group) thread of the warp would recompute the flow behind four gathers, a second
      // memory round trip in front of the corner loads: there the separate (2-channel) resize launch is faster - 1080p step
      // 45.8 -> 45.5 ms, warp class 3.18 -> 2.90 + 0.06 ms (profiles/r03_fuse_ab.log).  Same arithmetic either way.
      const bool fuse_up = (h->opt_fuse & FUSE_FLOW_UP) && (int64_t)Hl * Wl < 100000;
      if (!fuse_up) {
        OpDesc up;
        up.kind = OP_FLOW_UP; up.tag = tg + ":resize2x";
        up.in = view(v[l + 1], 0, 0, 2); up.out = view(vup[l], 0, 0, 2);
        up.NB = N2; up.H = HL(l + 1); up.W = WL(l + 1);
        up.bytes = 4.0 * N2 * Hl * Wl * 2 * 1.25;
        P->ops.push_back(up);
      }
      // Both directions in ONE launch (batch n = d * B + b, like every other op of the estimator): direction d warps the OTHER
      // image's features, i.e. the source batch is rotated by B (pyramid_flow_estimator.py:150-158 runs the two directions as
      // two calls; the arithmetic per pixel is the same).
      // Sequence plan: one launch per direction, the other image's features one offset of T images away (no batch rotation).
      for (int d = 0; d < (seq ? 2 : 1); ++d) {
        if (seq)
          warp(tg + ":warp_d" + std::to_string(d), view(feat[l], d ? i0 : i1, 0, fc[l]), view(vup[l], d * B, 0, 2),
               view(warped[l], d * B, 0, fc[l]), B, Hl, Wl, 1.f);
        else {
          warp(tg + ":warp_d01", view(feat[l], 0, 0, fc[l]), view(vup[l], 0, 0, 2), view(warped[l], 0, 0, fc[l]), N2, Hl, Wl, 1.f);
          P->ops.back().src_brot = B;
        }
        if (fuse_up) {
          // tf.image.resize(2 * v) (pyramid_flow_estimator.py:155) inside the warp: the flow of this level is computed
          // from the coarser level's v by every thread of a pixel and stored once (to vup, which v = res + up reads)
          OpDesc& w = P->ops.back();
          w.tag += "+resize2x";
          w.in2 = View();
          w.in3 = view(v[l + 1], d * B, 0, 2);
          w.out2 = view(vup[l], d * B, 0, 2);
        }
      }
    }
    View cur = scratch(fp[0], nf);
    if (!seq) {
      SegDesc sa = seg(view(feat[l], 0, 0, fc[l])), sb = seg(view(coarsest ? feat[l] : warped[l], 0, 0, fc[l]));
      if (coarsest) { sb.boff = B; sb.bmod = N2; }   // the other image's features
      conv(tg, prefix + "/conv_0", {sa, sb}, cur, N2, Hl, Wl, true);
    } else {
      // [features of image a | (warped) features of image b] per direction d: a = image d of pair-tile p, b = its image 1 - d
      // (coarsest level) or warped[d B + p]; the two halves of the output are the 2B batch of the pair plan
      for (int d = 0; d < 2; ++d) {
        SegDesc a = seg(view(feat[l], d ? i1 : i0, 0, fc[l]));
        SegDesc b = seg(coarsest ? view(feat[l], d ? i0 : i1, 0, fc[l]) : view(warped[l], d * B, 0, fc[l]));
        View o = cur;
        o.off += (int64_t)d * B * Hl * Wl * nf;
        conv(tg + ":d" + std::to_string(d), prefix + "/conv_0", {a, b}, o, B, Hl, Wl, true);
      }
    }
    int which = 0;
    for (int j = 1; j < nconv; ++j) {
      View nxt = scratch(fp[which ^ 1], nf);
      conv(tg, prefix + "/conv_" + std::to_string(j), {seg(cur)}, nxt, N2, Hl, Wl, true);
      cur = nxt; which ^= 1;
    }
    // the two 1x1 convolutions behind the 3x3 stack -> res[l]
    const int64_t M = (int64_t)N2 * Hl * Wl;
    const std::string l3 = prefix + "/conv_" + std::to_string(nconv), l4 = prefix + "/conv_" + std::to_string(nconv + 1);
    if ((nf / 2) % 32 == 0) {
      View hid = scratch(fp[2], nf / 2);
      conv(tg, l3, {seg(cur)}, hid, N2, Hl, Wl, true);
      conv_pw(tg, l4, hid, view(res[l], 0, 0, 2), M, false);
    } else {  // nf / 2 == 16: both 1x1 convs in one kernel, the 16-channel hidden layer stays in registers
      const LayerPack &L3 = layer(l3), &L4 = layer(l4);
      OpDesc op;
      op.kind = OP_FLOW_HEAD; op.tag = tg + ":" + l3 + "+conv_" + std::to_string(nconv + 1);
      op.in = cur; op.out = view(res[l], 0, 0, 2); op.n = M; op.Ctot = nf;
      op.w_off = L3.w_off; op.b_off = L3.b_off; op.w2_off = L4.w_off; op.b2_off = L4.b_off;
      op.flops = 2.0 * op.n * (nf * 16 + 16 * 2); op.bytes = 4.0 * op.n * (nf + 2);
      P->ops.push_back(op);
    }
    if (!coarsest && (h->opt_fuse & FUSE_FLOW_ADD)) {   // v = res + up in the epilogue of whichever head was pushed (coarsest level: v is res)
      OpDesc& head = P->ops.back();
      head.tag += "+v=res+up";
      head.in2 = view(vup[l], 0, 0, 2); head.out2 = view(v[l], 0, 0, 2);
    } else if (!coarsest) {
      OpDesc ad;
      ad.kind = OP_FLOW_ADD; ad.tag = tg + ":v=res+up";
      ad.in = view(res[l], 0, 0, 2); ad.in2 = view(vup[l], 0, 0, 2); ad.out = view(v[l], 0, 0, 2);
      ad.n = M * 2; ad.bytes = 4.0 * ad.n * 3;
      P->ops.push_back(ad);
    }
    // levels >= 4 read features of subtrees >= 1 only (level 3 needs the last stage of the level-0 subtree)
    if (l >= 4) to_lane(first_op, 1);
  }

  // warp to t = 0.5 and build the aligned pyramid (interpolator.py:153-183), level l.
  // util.flow_pyramid_synthesis recomputes exactly the v sequence above, so v is reused.
  // image s is sampled with the flow of the opposite direction: image 0 <- backward flow (d=1).
  // Emitted coarse to fine and on the side stream: level l only needs v[l], which the flow estimator finishes
  // early for the coarse levels; the level-0 warps (60 % of the warp bytes, HBM bound) then overlap the
  // fusion convolutions (matrix-pipe bound) of the main stream.
  void emit_align(int l) {
    const size_t first_op = P->ops.size();
    const std::string tg = "align_l" + std::to_string(l);
    // Planar level: the planes of image 0 and image 1 follow each other, i.e. they are ONE [2B][H][W][C] array - both feature warps
    // in one launch (batch n = s * B + b; image s is sampled with the flow of the opposite direction: the flow batch is rotated by B).
    // (sequence plans: image 1 is not at +B, so both the pair launch and the fused misc16 warp are out - the per-image branch)
    const bool pair = P->bufs[aligned[l]].planar > 0 && !seq;
    const bool misc16 = (h->opt_fuse & FUSE_MISC16) && !seq;
    if (pair) {
      warp(tg + ":warp_feat01", view(feat[l], 0, 0, fc[l]), view(v[l], 0, 0, 2), aligned_part(aligned[l], 0, fc[l]), N2, HL(l), WL(l), 0.5f);
      P->ops.back().flow_brot = B;
    }
    for (int s = 0; s < 2; ++s) {
      View fl = view(v[l], (1 - s) * B, 0, 2);
      if (!pair)
        warp(tg + ":warp_feat" + std::to_string(s), view(feat[l], s ? i1 : i0, 0, fc[l]), fl,
             aligned_part(aligned[l], s, fc[l]), B, HL(l), WL(l), 0.5f);
      if (!misc16)
        warp(tg + ":warp_img" + std::to_string(s), view(img[l], s ? i1 : i0, 0, 3), fl,
             sub(aligned_part(aligned[l], 2, fc[l]), 3 * s, 3), B, HL(l), WL(l), 0.5f, false);
    }
    if (misc16) {
      // the sixteen miscellaneous channels [warp(img0) 3 | warp(img1) 3 | 0.5 bflow 2 | 0.5 fflow 2 | 0 x 6] ride in the second
      // feature warp of the level as one more channel slice (one full 64-byte line per pixel and store)
      OpDesc& w = P->ops.back();
      w.tag += "+misc16";
      if (pair) w.misc_nb = B;
      w.img_in = view(img[l], 0, 0, 3);             // [2B]: image 0, image 1
      w.img_out = aligned_part(aligned[l], 2, fc[l]);
      w.pack_b = view(v[l], B, 0, 2);   // backward flow (d = 1): samples image 0
      w.pack_f = view(v[l], 0, 0, 2);   // forward flow  (d = 0): samples image 1
      w.bytes += 4.0 * B * HL(l) * WL(l) * 12.0;   // both 3-channel images, read + written (SURVEY 8d counts the image with the features)
    } else {
      OpDesc pk;
      pk.kind = OP_PACK_FLOW; pk.tag = tg + ":flows";
      pk.in = view(v[l], B, 0, 2);   // backward flow (d = 1)
      pk.in2 = view(v[l], 0, 0, 2);  // forward flow  (d = 0)
      pk.out = sub(aligned_part(aligned[l], 2, fc[l]), 6, 10);
      pk.n = (int64_t)B * HL(l) * WL(l); pk.bytes = 4.0 * pk.n * 14;
      P->ops.push_back(pk);
    }
    to_lane(first_op, 1);
  }

  // fusion decoder (fusion.py:103-140), level i: `net` (the level below, upsampled) and aligned[i] -> the new `net`
  void emit_fusion(int i, int lane) {
    const size_t first_op = P->ops.size();
    const std::string tg = "fusion_l" + std::to_string(i);
    const std::string base = "fusion/convs_" + std::to_string(i);
    conv(tg, base + "_0", {seg(net, 1)}, view(fu_u[i], 0, 0, ff[i]), B, HL(i), WL(i), false);
    const SegDesc up = seg(view(fu_u[i], 0, 0, ff[i]));
    if (P->bufs[aligned[i]].planar)
      conv(tg, base + "_1", {seg(aligned_part(aligned[i], 0, fc[i])), seg(aligned_part(aligned[i], 1, fc[i])), seg(aligned_part(aligned[i], 2, fc[i])), up},
           view(fu_a[i], 0, 0, ff[i]), B, HL(i), WL(i), true);
    else
      conv(tg, base + "_1", {seg(view(aligned[i], 0, 0, 2 * fc[i] + 16)), up}, view(fu_a[i], 0, 0, ff[i]), B, HL(i), WL(i), true);
    conv(tg, base + "_2", {seg(view(fu_a[i], 0, 0, ff[i]))}, view(fu_b[i], 0, 0, ff[i]), B, HL(i), WL(i), true);
    net = view(fu_b[i], 0, 0, ff[i]);
    to_lane(first_op, lane);
  }

  // RGB head (fusion.py:138-140): a 1x1 convolution of the last decoder layer.  Fused (FUSE_RGB_HEAD) into that
  // layer's epilogue when it runs on a Winograd kernel with 64 output channels and no split: the 64-channel
  // activation (566 MB per 1080p step) is then neither written nor read back.
  void emit_rgb_head() {
    OpDesc& last = P->ops.back();
    const LayerPack& LO = layer("fusion/output_conv");
    if ((h->opt_fuse & FUSE_RGB_HEAD) && last.kind == OP_CONV && kConvFamily[last.family].fused_shape >= 0 && last.Cout == 64 && last.ksplit <= 1 &&
        last.out2.buf < 0 && LO.cout <= 4 && LO.cin == 64) {
      last.tag += "+output_conv";
      last.pw_out = view(out_buf, 0, 0, 3); last.pw_cout = LO.cout;
      last.w2_off = LO.w_off; last.b2_off = LO.b_off;
      last.tile = conv_tile(last.family, kConvFamily[last.family].fused_shape, true);
      last.flops += 2.0 * (double)B * H0 * W0 * LO.cout * LO.cin;
      last.bytes = 4.0 * (double)B * H0 * W0 * (64 + LO.cout);
    } else {
      conv_pw("fusion_out", "fusion/output_conv", net, view(out_buf, 0, 0, 3), (int64_t)B * H0 * W0, false);
    }
  }

  int build(int B_, int H_, int W_, int T_, int slots, int left, int right, bool extract) {
    const film_config& c = h->cfg;
    B = B_; H0 = H_; W0 = W_; T = T_;
    NL = c.pyramid_levels; FL = c.fusion_pyramid_levels;
    seq = T > 0;
    N2 = 2 * B;
    NI = seq ? B + T : N2;
    i0 = 0; i1 = seq ? T : B;
    NE = NI; e0 = 0;
    if (slots > 0) {   // stream plan: the right frame (the pair's image 1) is extracted into slot `right`, image 0 waits in slot `left`
      if (slots < 2 || left < 0 || right < 0 || left >= slots || right >= slots || left == right || B != T)
        return fail(h, FILM_ERR_INVALID, "a stream plan has two different slots out of its %d and one pair of its tiles", slots);
      NI = slots * T;
      i0 = left * T; i1 = right * T;
      NE = T; e0 = i1;
    }
    fc = feature_channels(c);
    ff = fusion_filters(c);
    P->B = B; P->H = H0; P->W = W0; P->tiles = T;
    P->slots = slots; P->right = slots > 0 ? right : -1; P->left = slots > 0 ? left : -1; P->extract = extract;
    add_buffers();
    emit_image_pyramids();
    for (int i = 0; i < NL; ++i) emit_extractor(i);
    // an orientation that extracts nothing: the extraction is emitted all the same - its split-K regions are part of the workspace
    // every orientation shares - and dropped again BEFORE the lanes are analysed, so no remaining op waits for one of them
    if (slots > 0 && !extract) P->ops.clear();
    P->n_extract = P->ops.size();
    for (int l = NL - 1; l >= 0; --l) emit_flow(l);
    // Option "lanes" >= 2 (NOT the default - measured 2 % slower, see opt_lanes), large frames: the COARSE decoder levels (>= 2) join the side stream right behind the
    // aligned levels they read - fusion level i only needs aligned[i], aligned[i + 1] / the level above, i.e. the flow
    // of level i, which the estimator finishes while it still has levels i - 1 .. 0 to go.  Their matrix-bound
    // convolutions then run beside the estimator's chain of HBM-bound warps, 1x1 heads and short launches on the main
    // stream instead of behind it; the fine levels (1, 0) stay on the main stream, where the level-0 warps of the side
    // stream overlap them as before.  Small frames keep the decoder behind the estimator (latency bound).
    const bool early_fusion = h->opt_lanes >= 2 && ((int64_t)H0 * W0 > 512 * 512 || h->opt_lanes >= 3) && FL >= 4;   // 3: test knob, any frame size
    net = view(aligned[FL - 1], 0, 0, 2 * fc[FL - 1] + 16);
    emit_align(FL - 1);
    if (early_fusion) {
      for (int i = FL - 2; i >= 0; --i) {
        emit_align(i);
        if (i >= 2) emit_fusion(i, 1);
      }
      for (int i = std::min(FL - 2, 1); i >= 0; --i) emit_fusion(i, 0);
    } else {
      for (int i = FL - 2; i >= 0; --i) emit_align(i);
      for (int i = FL - 2; i >= 0; --i) emit_fusion(i, 0);
    }
    emit_rgb_head();
    if (bad) return fail(h, FILM_ERR_INVALID, "%s", bad_msg.c_str());
    P->arena_floats = cursor;   // the split-K partial-sum regions are added while the ops are emitted
    analyze_lanes();
    return FILM_OK;
  }

  // ---- cross-lane dependencies from buffer overlap -------------------------------------------------------------
  struct Access { int buf; int c0, c1; };  // channels [c0, c1) of every pixel of a buffer (scratch: everything)
  Access access(const View& v) const {
    const Buffer& b = P->bufs[v.buf];
    if (b.C == 0 || v.stride != b.C) return {v.buf, 0, 1 << 30};  // scratch, or a reinterpreted view: whole buffer
    const int c0 = (int)((v.off - b.off) % b.C);
    return {v.buf, c0, c0 + v.C};
  }
  static bool overlap(const Access& a, const Access& b) { return a.buf == b.buf && a.c0 < b.c1 && b.c0 < a.c1; }
  void accesses(const OpDesc& op, std::vector<Access>& rd, std::vector<Access>& wr) const {
    std::vector<const View*> r, w;
    op_views(op, r, w);
    rd.clear(); wr.clear();
    for (const View* v : r) rd.push_back(access(*v));
    for (const View* v : w) wr.push_back(access(*v));
  }
  // For every op: the LAST op of the other lane it conflicts with (RAW, WAR or WAW on overlapping channels of a
  // buffer).  Waiting for the last one is enough: a lane executes in program order.  For the same reason a wait is
  // dropped when the lane has already waited for that op or a later one of the other lane: every op of a lane is then
  // waited for at most ONCE by the other lane, i.e. a graph node has at most two children (its lane successor and one
  // cross-lane waiter).  That is not only tidier: the graph replay of HIP 7.0/7.2 starts a node whose ONLY parent
  // already has >= 5 earlier-captured children without waiting for that parent
  // (tools/experiments/graph_single_parent_race.hip).
  void analyze_lanes() {
    const size_t n = P->ops.size();
    std::vector<std::vector<Access>> rd(n), wr(n);
    for (size_t i = 0; i < n; ++i) accesses(P->ops[i], rd[i], wr[i]);
    long waited[2] = {-1, -1};   // per lane: the latest op of the other lane it has waited for
    for (size_t j = 0; j < n; ++j) {
      OpDesc& oj = P->ops[j];
      const int lj = oj.lane ? 1 : 0;
      for (size_t ii = j; ii-- > 0;) {
        const OpDesc& oi = P->ops[ii];
        if ((oi.lane ? 1 : 0) == lj) continue;
        if ((long)ii <= waited[lj]) break;   // ordered already (and so is everything before it)
        bool hit = false;
        for (const Access& w : wr[ii]) {
          for (const Access& r : rd[j]) hit |= overlap(w, r);
          for (const Access& w2 : wr[j]) hit |= overlap(w, w2);
        }
        for (const Access& r : rd[ii])
          for (const Access& w2 : wr[j]) hit |= overlap(r, w2);
        if (hit) { oj.xdeps.push_back((int)ii); P->ops[ii].signal = true; waited[lj] = (long)ii; break; }
      }
    }
  }
};

}  // namespace

int plan_build(film_t* h, Plan* P, int B, int H, int W, int tiles, int slots, int left, int right, bool extract) {
  Planner pl{h, P};
  return pl.build(B, H, W, tiles, slots, left, right, extract);
}

// The conv kernels other than conv_wino43_kernel address their inputs with 32-bit byte offsets from the start of the
// buffer (buffer loads): every activation buffer THEY read must stay below 4 GiB.  conv_wino43_kernel addresses relative
// to the workgroup's own halo rows and every other kernel with 64-bit pointers, so the large levels of a large frame
// (F(4,3) layers only: an untiled 4K frame has 4.4-5 GB level-0 buffers) are not limited.  Largest limited buffer of a
// B = 1 plan, in bytes (buffers scale linearly with the batch; the kernel family of a layer does not depend on it).
// The whole buffer bounds what a kernel addresses through a view that starts inside it (a sequence plan's view of the
// images from `tiles` on: its resource begins at the view and reaches no further than the buffer's end).
int64_t limited_buffer_bytes(const Plan* P) {
  int64_t mx = 1;
  for (const OpDesc& op : P->ops) {
    if (op.kind != OP_CONV || op.family == FAM_W43 || op.family == FAM_W2D) continue;
    for (int i = 0; i < op.nseg; ++i) mx = std::max(mx, P->bufs[op.seg[i].v.buf].floats * (int64_t)sizeof(float));
  }
  return mx;
}

namespace {
// one JSON object: "key":value pairs, comma-separated in the order they are added ("{" goes in front of the first key; the owner writes "}")
struct JsonObject {
  std::ostringstream& o;
  const char* sep = "{";
  std::ostringstream& key(const char* k) { o << sep << "\"" << k << "\":"; sep = ","; return o; }
  template <class T> void num(const char* k, const T& v) { key(k) << v; }
  void str(const char* k, const std::string& v) { key(k) << "\"" << v << "\""; }
  template <class T, class F> void list(const char* k, const T* a, size_t n, F each) {   // "key":[each(a[0]),each(a[1]),...]
    key(k) << "[";
    for (size_t i = 0; i < n; ++i) { o << (i ? "," : ""); each(a[i]); }
    o << "]";
  }
  template <class T> void ints(const char* k, const T* a, size_t n) { list(k, a, n, [&](const T& v) { o << v; }); }
  template <class T, class F> void objects(const char* k, const T* a, size_t n, F fill) {   // ... of objects: fill(object, a[i]) adds the pairs
    list(k, a, n, [&](const T& v) { JsonObject e{o}; fill(e, v); o << "}"; });
  }
  void view(const char* k, const View& v, const Plan& P) {
    JsonObject j{key(k)};
    j.str("buf", v.buf >= 0 ? P.bufs[v.buf].name : std::string(""));
    j.num("off", v.off); j.num("stride", v.stride); j.num("C", v.C);
    o << "}";
  }
};

void json_op(JsonObject& j, const OpDesc& op, const Plan& P) {
  const FamilyCodes fc = family_codes(op.family);
  j.str("kind", kKindName[op.kind]); j.str("tag", op.tag); j.num("NB", op.NB); j.num("H", op.H); j.num("W", op.W);
  j.num("ksize", op.ksize); j.num("leaky", op.leaky); j.num("Cout", op.Cout); j.num("Ctot", op.Ctot); j.num("tile", op.tile);
  // the weight copies of the layer, and behind the copy of a kernel family the code that says whether the op runs on it
  j.num("w_off", op.w_off); j.num("b_off", op.b_off); j.num("wf4_off", op.wf4_off);
  j.num("wh_off", op.wh_off); j.num("halo", fc.halo); j.num("ws_off", op.ws_off); j.num("split", fc.split);
  j.num("ww_off", op.ww_off); j.num("wx_off", op.wx_off); j.num("wfx_off", op.wfx_off); j.num("w43_off", op.w43_off); j.num("w2d_off", op.w2d_off);
  j.num("wino", fc.wino); j.num("fold", op.fold); j.num("ksplit", op.ksplit);
  j.num("py", op.py); j.num("px", op.px); j.num("ftaps", op.ftaps); j.ints("tdy", op.tdy, 4); j.ints("tdx", op.tdx, 4);   // (always 0: no plan has a single-phase fold)
  j.ints("fold_woff", op.fold_woff, 4); j.num("lane", op.lane); j.ints("xdeps", op.xdeps.data(), op.xdeps.size());
  j.num("w2_off", op.w2_off); j.num("b2_off", op.b2_off); j.num("c3", fc.c3);
  j.num("fscale", op.fscale); j.num("src_brot", op.src_brot); j.num("flow_brot", op.flow_brot); j.num("misc_nb", op.misc_nb); j.num("n", op.n);
  j.num("flops", op.flops); j.num("bytes", op.bytes);
  j.view("in", op.in, P); j.view("in2", op.in2, P); j.view("in3", op.in3, P); j.view("out2", op.out2, P); j.view("pw_out", op.pw_out, P); j.num("pw_cout", op.pw_cout);
  j.view("img_in", op.img_in, P); j.view("img_out", op.img_out, P); j.view("pack_b", op.pack_b, P); j.view("pack_f", op.pack_f, P); j.view("out", op.out, P);
  j.objects("segs", op.seg, op.nseg, [&](JsonObject& s, const SegDesc& g) {
    s.view("v", g.v, P); s.num("boff", g.boff); s.num("bmod", g.bmod); s.num("up", g.up);
  });
  // the tile codes the autotuner and film_debug_run_op would try for the op (a plan-only handle can say them: they depend on the descriptor alone)
  const std::vector<int> cands = op.kind == OP_CONV ? conv_candidates(op) : std::vector<int>();
  j.ints("cands", cands.data(), cands.size());
}
}  // namespace

std::string plan_json(film_t* h, const Plan& P, bool orientation_keys) {
  std::ostringstream o;
  JsonObject j{o};
  j.num("B", P.B); j.num("H", P.H); j.num("W", P.W);
  if (P.right >= 0) {
    j.str("kind", "stream"); j.num("tiles", P.tiles);
    if (orientation_keys) { j.num("slots", P.slots); j.num("left", P.left); j.num("right", P.right); }
    else j.num("slot", P.right);
    j.num("n_extract", P.n_extract);
  }
  else if (P.tiles > 0) { j.str("kind", "sequence"); j.num("n_pairs", P.B / P.tiles); j.num("tiles", P.tiles); }
  j.num("arena_floats", P.arena_floats); j.num("offset32_buffer_bytes", limited_buffer_bytes(&P)); j.num("packed_floats", h->packed_floats);
  j.objects("buffers", P.bufs.data(), P.bufs.size(), [](JsonObject& e, const Buffer& b) {
    e.str("name", b.name); e.num("off", b.off); e.num("N", b.N); e.num("H", b.H); e.num("W", b.W); e.num("C", b.C); e.num("floats", b.floats); e.num("planar", b.planar);
  });
  j.objects("layers", h->layers.data(), h->layers.size(), [](JsonObject& e, const LayerPack& L) {
    e.str("name", L.name); e.num("kh", L.kh); e.num("kw", L.kw); e.num("cin", L.cin); e.num("cout", L.cout); e.num("ctot", L.ctot());
    e.num("w_off", L.w_off); e.num("b_off", L.b_off); e.num("wh_off", L.wh_off); e.num("ws_off", L.ws_off); e.num("ww_off", L.ww_off); e.num("wx_off", L.wx_off);
  });
  j.objects("ops", P.ops.data(), P.ops.size(), [&](JsonObject& e, const OpDesc& op) { json_op(e, op, P); });
  o << "}";
  return o.str();
}

}  // namespace film_internal
