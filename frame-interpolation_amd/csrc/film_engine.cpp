// film_engine.cpp -- C-ABI (include/film_hip.h) of the MI355X FILM inference engine: handle lifetime, the option table, the JSON queries,
// tiling, staging and chunking of film_forward / film_interpolate / film_interpolate_sequence, the host-buffer pipeline, film_get_tap and the
// debug entry points, and the helpers the entry points of film_stream.cpp (the frame streams, film_stream_*) share with these (tile_geometry,
// check_pix, need_device, pick_stream).  The executor lives in film_exec.cpp, the autotuner in film_tune.cpp, the plan cache in film_plans.cpp, the planner in
// film_planner.cpp, the layer table and the weight packer in film_layers.cpp, the shared structures in film_internal.h.
// There is no CPU execution path here: plan-only handles (device = -1) can pack weights and describe
// plans, every compute entry point needs a HIP device.
#include "film_internal.h"

namespace film_internal {

thread_local std::string g_create_error;

int fail(film_t* h, int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}

int copy_out_string(film_t* h, const std::string& s, char* buf, int64_t cap, int64_t* needed) {
  if (needed) *needed = (int64_t)s.size() + 1;
  if (!buf || cap < (int64_t)s.size() + 1) {
    if (!buf && needed) return FILM_OK;  // size query
    return fail(h, FILM_ERR_INVALID, "buffer too small: need %lld bytes", (long long)s.size() + 1);
  }
  memcpy(buf, s.c_str(), s.size() + 1);
  return FILM_OK;
}

// ---- what the entry points here and in film_stream.cpp share
// Geometry of a frame cut into block_h x block_w patches, each padded to a multiple of `align` (_pad_to_align, eval/interpolator.py:45-52).
// The two refusals are the reference's asserts (eval/interpolator.py:84-89), same messages.  tp->B, src, dst and the tile range are the caller's.
// Options "block_overlap_h" / "block_overlap_w" are resolved here, per axis of nb blocks of p pixels: one block has no overlap; -1 is
// min(pad0 / 2, p / 2), pad0 = the zero padding of a p-sized patch (the padded tile stays the same); else 2 o <= p is required.  A tile holds
// e = p + 2 o pixels from film_tile_origin and is padded to `align` like a patch (overlap 0: e = p, the patches of the reference).
int tile_geometry(film_t* h, int H, int W, int block_h, int block_w, int align, TileMapParams* tp) {
  const int bh = block_h > 0 ? block_h : 1, bw = block_w > 0 ? block_w : 1;
  if (H % bh) return fail(h, FILM_ERR_INVALID, "block_height=%d should evenly divide height=%d.", bh, H);
  if (W % bw) return fail(h, FILM_ERR_INVALID, "block_width=%d should evenly divide width=%d.", bw, W);
  tp->H = H; tp->W = W; tp->bh = bh; tp->bw = bw; tp->ph = H / bh; tp->pw = W / bw;
  struct Axis { const char* key; int nb, p, want; int *ov, *e, *T, *off; };
  const Axis axes[2] = {{"block_overlap_h", bh, tp->ph, h->opt_block_overlap_h, &tp->ovy, &tp->eh, &tp->TH, &tp->oy},
                        {"block_overlap_w", bw, tp->pw, h->opt_block_overlap_w, &tp->ovx, &tp->ew, &tp->TW, &tp->ox}};
  for (const Axis& a : axes) {
    const int pad0 = (align > 0 && a.p % align) ? align - a.p % align : 0;
    const int o = a.nb == 1 ? 0 : a.want < 0 ? std::min(pad0 / 2, a.p / 2) : a.want;
    if (2 * (int64_t)o > a.p)
      return fail(h, FILM_ERR_INVALID, "%s: twice the overlap (%d) must not exceed the patch size %d", a.key, o, a.p);
    const int e = a.p + 2 * o;
    const int pad = (align > 0 && e % align) ? align - e % align : 0;
    *a.ov = o; *a.e = e; *a.T = e + pad; *a.off = pad / 2;
  }
  return FILM_OK;
}
// The `pix` argument of the stream and debug entry points: a layout in bits 0-7 plus the colour flags of the Y'CbCr layouts (kPixLayouts and its
// look-ups: film_kernels.h).
// FILM_OK, or the refusal of a pix value for H x W frames (include/film_hip.h, film_stream_open)
int check_pix(film_t* h, int pix, int H, int W) {
  const int layout = pix_layout(pix), flags = pix & ~0xff;
  constexpr int known = FILM_YUV_BT601 | FILM_YUV_BT2020 | FILM_YUV_FULL;
  if (layout != FILM_PIX_F32 && layout != FILM_PIX_U8 && !pix_is_yuv(pix))
    return fail(h, FILM_ERR_INVALID, "bad pix layout %d: %s", layout, pix_layout_list(false).c_str());
  if (flags & ~known)
    return fail(h, FILM_ERR_INVALID, "bad pix 0x%x: unknown bits 0x%x set (flags: FILM_YUV_BT601 0x100, FILM_YUV_FULL 0x400, FILM_YUV_BT2020 0x2000)", (unsigned)pix,
                (unsigned)(flags & ~known));
  if (flags && !pix_is_yuv(pix))
    return fail(h, FILM_ERR_INVALID, "bad pix 0x%x: the colour flags belong to the Y'CbCr layouts, not to an RGB layout", (unsigned)pix);
  if ((flags & FILM_YUV_BT601) && (flags & FILM_YUV_BT2020))
    return fail(h, FILM_ERR_INVALID, "bad pix 0x%x: FILM_YUV_BT601 and FILM_YUV_BT2020 name two matrices", (unsigned)pix);
  const ChromaShift cs = pix_chroma_shift(pix);
  if (cs.sy && H > 0 && W > 0 && ((H | W) & 1))
    return fail(h, FILM_ERR_INVALID, "pix: 4:2:0 needs even sizes, got %d x %d", H, W);
  if (cs.sx && !cs.sy && H > 0 && W > 0 && (W & 1))
    return fail(h, FILM_ERR_INVALID, "pix: 4:2:2 needs an even width, got %d x %d", H, W);
  return FILM_OK;
}
// samples of one H x W frame of pixel type `pix` (S of "Scene cuts", include/film_hip.h), and its bytes
int64_t frame_samples(int pix, int H, int W) {
  const ChromaShift cs = pix_chroma_shift(pix);
  return pix_is_yuv(pix) ? (int64_t)H * W + 2 * (int64_t)(H >> cs.sy) * (W >> cs.sx) : (int64_t)H * W * 3;
}
size_t frame_bytes(int pix, int H, int W) { return (size_t)frame_samples(pix, H, W) * pix_sample_bytes(pix); }
// The refusals the compute entry points share (`fn`: the entry point); where they stand among its other checks is the entry point's choice.
int need_device(film_t* h, const char* fn) {
  if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle: %s needs a HIP device (no CPU fallback)", fn);
  if (!h->finalized) return fail(h, FILM_ERR_STATE, "film_finalize has not been called");
  return FILM_OK;
}
hipStream_t pick_stream(film_t* h, int mem_kind, void* stream) {
  // stream == NULL: host buffers -> the handle's own (non-blocking) stream, synchronised before returning;
  // device buffers -> the NULL (legacy default) stream, i.e. ordered with the caller's default-stream work
  // (torch's default stream IS the NULL stream, and its handle is 0).
  return stream ? (hipStream_t)stream : (mem_kind == FILM_MEM_DEVICE ? (hipStream_t) nullptr : h->stream);
}

// Chunk size for n independent units with at most maxc per invocation: the largest divisor of n in (maxc / 2, maxc] if
// there is one, so that every invocation runs the SAME cached plan (16 * 2^k tiles of a 4K recursion with maxc = 15 ->
// chunks of 8, never a 15 + 1 split that would build, tune and capture a second plan for the remainder); else maxc.
int balanced_chunk(int n, int maxc) {
  if (n <= maxc) return n;
  for (int c = maxc; 2 * c > maxc; --c)
    if (n % c == 0) return c;
  return maxc;
}
// The retry rule of the chunk loops: a chunk of more than one unit whose workspace did not fit (FILM_ERR_NOMEM from get_plan: nothing was
// launched) is halved, and the caller goes again from the same place.
bool halve_on_nomem(int rc, int* chunk) {
  if (rc != FILM_ERR_NOMEM || *chunk <= 1) return false;
  *chunk = (*chunk + 1) / 2;
  return true;
}

}  // namespace film_internal

using namespace film_internal;

namespace {

// ---- options: one row per key of film_set_option (what each value means: include/film_hip.h; the measurements behind the defaults: beside the
// opt_* fields in film_internal.h).  A value is range-checked, refused where it needs a kernel family this library does not hold, normalised and
// stored; the plans carry the op list, the buffer layout, the lanes and the kernel and tile of every op, so a CHANGED value of an option that
// decides any of those drops them.
enum OptNorm { AS_IS, BOOL, NONNEG, LOW5 };   // stored: value | value != 0 | max(value, 0) | value & 31
// a row reads: key, field, norm, drops_plans [, lo, hi, refusal [, family, need_lo, need_hi, family_refusal]]
struct OptionRow {
  const char* key;
  int film_t::*field;   // nullptr: "pack_groups" stores nothing - it packs the weight layout groups 1..value of a finalized handle now
  OptNorm norm;
  bool drops_plans;
  int64_t lo = 0, hi = 0;
  const char* refusal = nullptr;          // of a value outside lo..hi (nullptr: every value is accepted)
  ConvFamily family = FAM_BUF;
  int need_lo = 0, need_hi = 0;
  const char* family_refusal = nullptr;   // of a stored value in need_lo..need_hi when `family` is not built (nullptr: no such values; %d = the value)
};
constexpr OptionRow kOptions[] = {
    {"graph", &film_t::opt_graph, AS_IS, false, 0, 2, "graph: 0 (one stream, eager), 1 (hipGraph replay) or 2 (two lanes, eager: the default)"},
    {"profile", &film_t::opt_profile, BOOL, false},
    {"autotune", &film_t::opt_autotune, BOOL, false},
    {"max_batch", &film_t::opt_max_batch, NONNEG, false},
    {"host_overlap", &film_t::opt_host_overlap, BOOL, false},
    {"block_overlap_h", &film_t::opt_block_overlap_h, AS_IS, false, -1, 65535, "block_overlap_h: -1 (what the align padding of a tile holds) or 0 .. 65535 rows"},
    {"block_overlap_w", &film_t::opt_block_overlap_w, AS_IS, false, -1, 65535, "block_overlap_w: -1 (what the align padding of a tile holds) or 0 .. 65535 columns"},
    {"stream_times", &film_t::opt_stream_times, AS_IS, false, 1, kMaxStreamTimes, "stream_times: 1 .. 6 (a primed push of a stream opened with T writes 2^T - 1 frames)"},
    {"scene_cut", &film_t::opt_scene_cut, AS_IS, false, 0, 1000, "scene_cut: 0 (off) or 1 .. 1000 permille of the histogram distance"},
    {"dup_hi", &film_t::opt_dup_hi, AS_IS, false, -1, 16320, "dup_hi: -1 (off) or 0 .. 16320, the largest 8 x 8 block SAD of a duplicate frame in 8-bit code units"},
    {"dup_lo", &film_t::opt_dup_lo, AS_IS, false, 0, 16320, "dup_lo: 0 .. 16320, the block SAD in 8-bit code units above which a block counts as changed"},
    {"dup_frac", &film_t::opt_dup_frac, AS_IS, false, 0, 1000, "dup_frac: 0 .. 1000 permille of a plane's blocks that may count as changed in a duplicate frame"},
    {"tune_ms", &film_t::opt_tune_ms, NONNEG, false},
    {"splitk", &film_t::opt_splitk, BOOL, true},
    {"pack_groups", nullptr, AS_IS, false, 1, 4, "pack_groups: 1 .. 4"},
    {"fuse", &film_t::opt_fuse, LOW5, true},
    {"fold2x2", &film_t::opt_fold2x2, AS_IS, true, 0, 2, "fold2x2: 0, 1 or 2"},
    {"planar", &film_t::opt_planar, BOOL, true},
    {"winograd", &film_t::opt_wino, AS_IS, true, 0, 3, "winograd: 0, 1, 2 or 3", FAM_WINO, 2, 2,
     "winograd = 2 (F(2,3) kernel on every level) needs a library built with FILM_EXTRA_FAMILIES=1"},
    {"halo_all", &film_t::opt_halo_all, BOOL, true, 0, 0, nullptr, FAM_HALO, 1, 1, "halo_all needs a library built with FILM_EXTRA_FAMILIES=1"},
    {"lanes", &film_t::opt_lanes, AS_IS, true, 0, 3, "lanes: 0, 1, 2 or 3"},
    {"wino2d", &film_t::opt_wino2d, AS_IS, true, 0, 2, "wino2d: 0, 1 or 2"},
    {"w2d_small_px", &film_t::opt_w2d_small_px, AS_IS, true, 0, 1 << 30, "w2d_small_px: pixels per image, 0 = never"},
    {"w2d_min_px", &film_t::opt_w2d_min_px, AS_IS, true, 1, 1 << 30, "w2d_min_px: pixels per image"},
    {"w2d_splitk", &film_t::opt_w2d_splitk, AS_IS, true, 0, 16, "w2d_splitk: 0 (off), 1 (default rule) or 2..16 (A/B: the cap on levels of <= 1024 pixels)"},
    {"w2d_shape", &film_t::opt_w2d_shape, AS_IS, true, -1, W2D_SHAPES - 1, "w2d_shape: -1 (autotuned) or a Wino2dTile shape index"},
    {"fold4_shape", &film_t::opt_fold4_shape, AS_IS, true, -1, F4_4x32, "fold4_shape: -1 (autotuned) or a Fold4Tile shape index"},
    {"w43_shape", &film_t::opt_w43_shape, AS_IS, true, -1, 31, "w43_shape: -1 (autotuned) or a Wino43Tile shape index"},
    {"precision", &film_t::opt_precision, AS_IS, true, 0, 2, "precision: 0 (f32), 1 (bf16x6) or 2 (bf16x3)", FAM_SPLIT6, 1, 2,
     "precision %d (bf16 split modes) needs a library built with FILM_EXTRA_FAMILIES=1; this build runs fp32 MFMA only"},
};
constexpr bool option_rows_complete() {
  for (const OptionRow& o : kOptions)
    if ((o.lo < o.hi) != (o.refusal != nullptr) || ((o.family != FAM_BUF) != (o.family_refusal != nullptr))) return false;
  return true;
}
static_assert(option_rows_complete(), "a row with a range (a family) carries its refusal message, a row without leaves lo = hi (family = FAM_BUF)");

// The handle's staging buffer in HBM (whole frames of the FILM_MEM_HOST entry points), grown on demand.
int ensure_stage(film_t* h, size_t bytes, hipStream_t s) {
  if (h->stage_bytes >= bytes) return FILM_OK;
  if (h->stage) { HIPCHK(h, hipStreamSynchronize(s)); HIPCHK(h, hipFree(h->stage)); h->stage = nullptr; h->stage_bytes = 0; }
  hipError_t e = hipMalloc(&h->stage, bytes);
  if (e != hipSuccess) return fail(h, FILM_ERR_NOMEM, "frame staging hipMalloc of %.1f MB failed", bytes * 1e-6);
  h->stage_bytes = bytes;
  return FILM_OK;
}
// Chunk of a sequence of n frame pairs of T tiles each, at most cap pair-tiles per plan: k consecutive pairs x nt tiles, i.e. (k + 1) * nt
// extracted image-tiles for k * nt pair-tiles.  Most pairs per extracted image = the largest k; ties go to the larger tile range (whole
// frames first).  Then balanced like balanced_chunk, so that the chunks of a sequence share one cached plan where they can.
// cap comes from the PAIR plan of one pair-tile: every buffer of a sequence plan of k * nt pair-tiles is at most the pair plan's of
// k * nt (images (k + 1) * nt <= 2 k nt, the flow estimator and the decoder the same), so its 4 GiB and arena limits hold here too.
void sequence_chunk(int n, int T, int cap, int* k, int* nt) {
  int bk = 0, bt = 1;
  for (int t = std::min(T, cap); t >= 1; --t) {
    const int kk = std::min(n, cap / t);
    if (kk > bk) { bk = kk; bt = t; }
  }
  *k = balanced_chunk(n, std::max(bk, 1));
  *nt = balanced_chunk(T, bt);
}
// Whole frames in HBM for a FILM_MEM_HOST call: the handle's staging buffer as [in_floats of inputs | the result].  open() grows it, upload()
// copies one input behind those before it and says where the work reads it, `out` is where the work leaves the result, finish() downloads it
// and waits.  A FILM_MEM_DEVICE call works on the caller's own pointers: upload() and `out` hand them back, finish() has nothing to do.
struct FrameStage {
  film_t* h; hipStream_t s; bool host;
  float* result; size_t out_floats;   // the caller's
  float* out = nullptr;
  size_t used = 0;
  int open(size_t in_floats) {
    out = result;
    if (!host) return FILM_OK;
    int rc = ensure_stage(h, (in_floats + out_floats) * sizeof(float), s);
    if (rc == FILM_OK) out = (float*)h->stage + in_floats;
    return rc;
  }
  int upload(const float* src, size_t floats, const float** dev) {
    *dev = src;
    if (!host) return FILM_OK;
    HIPCHK(h, hipMemcpyAsync((float*)h->stage + used, src, floats * sizeof(float), hipMemcpyHostToDevice, s));
    *dev = (float*)h->stage + used;
    used += floats;
    return FILM_OK;
  }
  int finish() {
    if (!host) return FILM_OK;
    HIPCHK(h, hipMemcpyAsync(result, out, out_floats * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return FILM_OK;
  }
};
// One chunk of a tiled call: every cut brings tiles [tile0, tile0 + ntiles) of the frame batch at `frames` into images slot .. of the plan's
// img0, the plan runs, every join takes images slot .. of its result into those tiles of the frame batch at `frames`.
template <class T> struct TileCopy { T* frames; int tile0, ntiles; int64_t slot; };
using Cut = TileCopy<const float>;
using Join = TileCopy<float>;
int run_chunk(film_t* h, Plan* P, TileMapParams tp, const std::vector<Cut>& cuts, const std::vector<Join>& joins, hipStream_t s) {
  const int64_t tile_floats = (int64_t)tp.TH * tp.TW * 3;
  for (const Cut& c : cuts) {
    tp.tile0 = c.tile0; tp.ntiles = c.ntiles; tp.src = c.frames; tp.dst = P->at("img0") + c.slot * tile_floats;
    HIPCHK(h, film_launch_cut_tiles(tp, FILM_PIX_F32, s));
  }
  int rc = run_plan(h, P, s);
  if (rc) return rc;
  for (const Join& j : joins) {   // (overlapped tiles: the joins of a frame add up in tile order on this one stream, chunk after chunk)
    tp.tile0 = j.tile0; tp.ntiles = j.ntiles; tp.src = P->at("out") + j.slot * tile_floats; tp.dst = j.frames;
    HIPCHK(h, film_launch_join_tiles(tp, s));
  }
  return FILM_OK;
}

int forward_chunk(film_t* h, const float* x0, const float* x1, int B, int H, int W, float* out, int mem_kind, void* stream) {
  HIPCHK(h, hipSetDevice(h->device));
  Plan* P = nullptr;
  int rc = get_plan(h, B, H, W, true, &P);
  if (rc) return rc;
  hipStream_t s = pick_stream(h, mem_kind, stream);
  const size_t in_bytes = (size_t)B * H * W * 3 * sizeof(float);
  const hipMemcpyKind kin = mem_kind == FILM_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const hipMemcpyKind kout = mem_kind == FILM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIPCHK(h, hipMemcpyAsync(P->at("img0"), x0, in_bytes, kin, s));
  HIPCHK(h, hipMemcpyAsync(P->at("img0") + (int64_t)B * H * W * 3, x1, in_bytes, kin, s));
  rc = run_plan(h, P, s);
  if (rc) return rc;
  HIPCHK(h, hipMemcpyAsync(out, P->at("out"), in_bytes, kout, s));
  if (mem_kind == FILM_MEM_HOST) HIPCHK(h, hipStreamSynchronize(s));
  return FILM_OK;
}

// film_interpolate with HOST buffers, one chunk, direct two-lane executor.  The reference's call is numpy -> numpy (eval/interpolator.py:152-209): the
// copies are part of it.  Instead of upload, upload, work, download:
//   main stream:  H2D x0 | tiles of x0 | first layers on x0's tiles ("head" parts 0) | wait E0 | the same layers on x1's tiles | ... the plan ... |
//                 last layer, first tile half | stitch first half, record E1 | last layer, second half | stitch | D2H second half
//   side stream:  (behind the tiles of x0) H2D x1 | tiles of x1 | record E0 | lane 1 of the plan ... | wait E1 | D2H first half
// The API calls are made in this order, so that it also holds for pageable memory, whose copies block the calling thread: the GPU works on x0
// while the host copies x1, and on the second half of the last layer while the host receives the first half of the frame.
// Splitting a convolution's batch into two launches cannot change a bit (batch_part).
int interpolate_host_pipeline(film_t* h, Plan* P, TileMapParams tp, const float* x0, const float* x1, float* out, float* st, size_t frame_bytes, hipStream_t s) {
  const int nt = P->B;
  const size_t nf = frame_bytes / sizeof(float);
  for (hipEvent_t& e : h->pipe_ev)
    if (!e) HIPCHK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  LanePipe lp;
  for (size_t i = 0; i < P->ops.size() && lp.head.size() < 2; ++i) {   // the leading main-lane convolutions that read nothing from the side lane
    const OpDesc& op = P->ops[i];
    if (op.lane == 1) continue;
    if (!batch_splittable(op, 2) || !op.xdeps.empty() || op.NB != 2 * nt) break;
    lp.head.push_back(i);
  }
  const OpDesc& last = P->ops.back();
  // the tiles of a frame are row-major blocks: the first half of the tiles = the upper half of the frame when there is one frame and an even
  // number of block rows
  lp.tail = tp.B == 1 && tp.bh % 2 == 0 && last.lane == 0 && last.pw_out.buf >= 0 && last.NB == nt && batch_splittable(last, 2) && P->ops.size() > lp.head.size() + 1 &&
            std::find(lp.head.begin(), lp.head.end(), P->ops.size() - 1) == lp.head.end();
  tp.tile0 = 0;
  lp.mid_tail = [&]() -> hipError_t {
    TileMapParams t2 = tp;
    t2.ntiles = nt / 2; t2.src = P->at("out"); t2.dst = st + 2 * nf;
    hipError_t e = film_launch_join_tiles(t2, s);
    if (e == hipSuccess) e = hipEventRecord(h->pipe_ev[1], s);
    return e;
  };
  // From here on copies and kernels are in flight on both streams: whatever fails, both are drained before the error goes back to the caller,
  // who may then free or reuse x1 / out (pinned memory makes the copies truly asynchronous).
  struct Drain {
    film_t* h; hipStream_t s; bool armed;
    ~Drain() { if (armed) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamSynchronize(s); } }
  } drain{h, s, true};
  HIPCHK(h, hipMemcpyAsync(st, x0, frame_bytes, hipMemcpyHostToDevice, s));
  tp.ntiles = nt; tp.src = st; tp.dst = P->at("img0");
  HIPCHK(h, film_launch_cut_tiles(tp, FILM_PIX_F32, s));
  HIPCHK(h, hipEventRecord(h->pipe_ev[0], s));
  HIPCHK(h, hipStreamWaitEvent(h->stream2, h->pipe_ev[0], 0));   // (the side stream: behind whatever `s` held before this call, too)
  for (size_t i : lp.head) HIPCHK(h, launch_op(batch_part(P->ops[i], 0, 2), P->arena, h->packed_dev, s));
  HIPCHK(h, hipMemcpyAsync(st + nf, x1, frame_bytes, hipMemcpyHostToDevice, h->stream2));
  tp.src = st + nf; tp.dst = P->at("img0") + (int64_t)nt * tp.TH * tp.TW * 3;
  HIPCHK(h, film_launch_cut_tiles(tp, FILM_PIX_F32, h->stream2));
  HIPCHK(h, hipEventRecord(h->pipe_ev[0], h->stream2));
  HIPCHK(h, hipStreamWaitEvent(s, h->pipe_ev[0], 0));
  const hipError_t le = issue_lanes(h, P, s, false, &lp);
  if (le != hipSuccess) return fail(h, FILM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(le));
  h->last_plan = P;
  const int64_t tile_floats = (int64_t)tp.TH * tp.TW * 3;
  if (lp.tail) {
    TileMapParams t2 = tp;
    t2.tile0 = nt / 2; t2.ntiles = nt - nt / 2; t2.src = P->at("out") + (int64_t)(nt / 2) * tile_floats; t2.dst = st + 2 * nf;
    HIPCHK(h, film_launch_join_tiles(t2, s));
    const size_t half = frame_bytes / 2;   // (one frame, an even number of block rows: the upper half of the rows)
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->pipe_ev[1], 0));
    HIPCHK(h, hipMemcpyAsync(out, st + 2 * nf, half, hipMemcpyDeviceToHost, h->stream2));
    HIPCHK(h, hipMemcpyAsync((char*)out + half, (const char*)(st + 2 * nf) + half, frame_bytes - half, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(h->stream2));
  } else {
    tp.tile0 = 0; tp.ntiles = nt; tp.src = P->at("out"); tp.dst = st + 2 * nf;
    HIPCHK(h, film_launch_join_tiles(tp, s));
    HIPCHK(h, hipMemcpyAsync(out, st + 2 * nf, frame_bytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(h, hipStreamSynchronize(s));
  drain.armed = false;
  return FILM_OK;
}

// The plan film_debug_arena / film_debug_run_op work on ("Debug / tests" in include/film_hip.h: one planned launch on a workspace the caller controls)
int debug_plan(film_t* h, int B, int H, int W, int tiles, Plan** P) {
  if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle has no device");
  if (!h->finalized) return fail(h, FILM_ERR_STATE, "weights are not finalized");
  if (tiles < 0 || (tiles > 0 && B % tiles)) return fail(h, FILM_ERR_INVALID, "tiles must be 0 (pair plan) or divide B (sequence plan)");
  HIPCHK(h, hipSetDevice(h->device));
  return get_plan(h, B, H, W, true, P, tiles);
}

// What film_debug_tile_map and film_debug_yuv_cut (`fn`) share behind their own argument checks: ONE cut (mode 0) or join (mode 1) of tiles
// [tile0, tile0 + ntiles) through the launchers every entry point uses.  The geometry and the range are checked before the device: a
// plan-only handle reports them like a device handle does.
int debug_tile_map(film_t* h, const char* fn, int mode, int pix, void* frames_dev, float* tiles_dev, int B, int H, int W, int align, int block_h,
                   int block_w, int tile0, int ntiles, hipStream_t s) {
  if (B < 1 || H < 1 || W < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  TileMapParams tp{};
  tp.B = B;
  int rc = tile_geometry(h, H, W, block_h, block_w, align, &tp);
  if (rc) return rc;
  const int64_t total = (int64_t)B * tp.bh * tp.bw;
  if (ntiles < 1 || tile0 < 0 || (int64_t)tile0 + ntiles > total)
    return fail(h, FILM_ERR_INVALID, "%s: tiles [%d, %lld) are no range of the %lld tiles of the batch", fn, tile0, (long long)tile0 + ntiles,
                (long long)total);
  if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle: %s needs a HIP device (no CPU fallback)", fn);
  HIPCHK(h, hipSetDevice(h->device));
  tp.tile0 = tile0; tp.ntiles = ntiles;
  if (mode == 0) {
    tp.src = static_cast<const float*>(frames_dev); tp.dst = tiles_dev;
    HIPCHK(h, film_launch_cut_tiles(tp, pix, s));
  } else {
    tp.src = tiles_dev; tp.dst = static_cast<float*>(frames_dev);
    HIPCHK(h, film_launch_join_tiles(tp, s));
  }
  return FILM_OK;
}

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int film_to_uint8(const float* src, unsigned char* dst, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!src || !dst))) return FILM_ERR_INVALID;
  return film_launch_to_uint8(src, dst, n, (hipStream_t)stream) == hipSuccess ? FILM_OK : FILM_ERR_HIP;
}

int film_frame_histogram(const void* frame_dev, int H, int W, int pix, uint32_t* hist_dev, void* stream) {
  if (!frame_dev || !hist_dev || H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || check_pix(nullptr, pix, H, W) != FILM_OK ||
      (reinterpret_cast<uintptr_t>(frame_dev) & 3))
    return FILM_ERR_INVALID;
  return film_launch_frame_histogram(frame_dev, H, W, pix, hist_dev, (hipStream_t)stream) == hipSuccess ? FILM_OK : FILM_ERR_HIP;
}

int film_frame_diff(const void* a_dev, const void* b_dev, int H, int W, int pix, int lo, uint64_t* out_dev, void* stream) {
  if (!a_dev || !b_dev || !out_dev || H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31) || check_pix(nullptr, pix, H, W) != FILM_OK ||
      ((reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(b_dev)) & 3) || lo < 0 || lo > 65535 || (reinterpret_cast<uintptr_t>(out_dev) & 7))
    return FILM_ERR_INVALID;
  return film_launch_frame_diff(a_dev, b_dev, H, W, pix, lo, out_dev, (hipStream_t)stream) == hipSuccess ? FILM_OK : FILM_ERR_HIP;
}

int film_to_yuv(const float* src, void* dst, int H, int W, int pix, void* stream) {
  if (!src || !dst || H < 1 || W < 1 || !pix_is_yuv(pix) || check_pix(nullptr, pix, H, W) != FILM_OK) return FILM_ERR_INVALID;
  if (pix_is_yuv10(pix) && (reinterpret_cast<uintptr_t>(dst) & 1)) return FILM_ERR_INVALID;   // (16-bit samples)
  return film_launch_rgb_to_yuv(src, dst, H, W, pix, (hipStream_t)stream) == hipSuccess ? FILM_OK : FILM_ERR_HIP;
}

int film_to_yuv420(const float* src, void* dst, int H, int W, int pix, void* stream) {
  if (!pix_chroma_shift(pix).sy) return FILM_ERR_INVALID;   // (the 4:2:0 layouts only, as ever; no Y'CbCr layout at all: film_to_yuv refuses it)
  return film_to_yuv(src, dst, H, W, pix, stream);
}

#ifndef FILM_SRC_ID
#define FILM_SRC_ID "unknown"
#endif
#ifdef FILM_EXTRA_FAMILIES
#define FILM_FLAVOUR "+extra"
#else
#define FILM_FLAVOUR ""
#endif
// "gfx950;film_hip r6;src=<sha1[:12] of csrc/ + include/film_hip.h>[+extra]": ties tune caches, bench lines and PMC summaries to the
// kernel sources they were produced with (film_hip/build.py source_id(), `make print-src-id`)
const char* film_version(void) { return "gfx950;film_hip r6;src=" FILM_SRC_ID FILM_FLAVOUR; }

int film_default_config(film_config* cfg) {
  if (!cfg) return FILM_ERR_INVALID;
  memset(cfg, 0, sizeof *cfg);
  cfg->pyramid_levels = 7; cfg->fusion_pyramid_levels = 5; cfg->specialized_levels = 3; cfg->sub_levels = 4;
  cfg->filters = 64;
  const int fcv[4] = {3, 3, 3, 3}, ffl[4] = {32, 64, 128, 256};
  for (int i = 0; i < 4; ++i) { cfg->flow_convs[i] = fcv[i]; cfg->flow_filters[i] = ffl[i]; }
  return FILM_OK;
}

int film_create(film_t** out, int device, const film_config* cfg) {
  if (!out) return fail(nullptr, FILM_ERR_INVALID, "out is NULL");
  *out = nullptr;
  std::unique_ptr<film_handle> h(new film_handle);
  if (cfg) h->cfg = *cfg; else film_default_config(&h->cfg);
  int rc = validate_config(h.get(), h->cfg);
  if (rc) { g_create_error = h->err; return rc; }
  h->device = device;
  h->plan_only = device < 0;
  if (!h->plan_only) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
      return fail(nullptr, FILM_ERR_NO_DEVICE, "no HIP device available (%s); libfilm_hip has no CPU fallback",
                  e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device >= ndev) return fail(nullptr, FILM_ERR_INVALID, "device %d out of range (%d devices)", device, ndev);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, FILM_ERR_HIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      return fail(nullptr, FILM_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess)
      return fail(nullptr, FILM_ERR_HIP, "hipStreamCreate failed");
  }
  build_layers(h.get());
  *out = h.release();
  return FILM_OK;
}

void film_destroy(film_t* h) {
  if (!h) return;
  drop_plans(h);   // (waits first: forwards may still be running on the caller's stream and on the side lane, and what they use must outlive them)
  stream_free(h);
  if (h->packed_dev) (void)hipFree(h->packed_dev);
  if (h->stage) (void)hipFree(h->stage);
  if (h->metrics_buf) (void)hipFree(h->metrics_buf);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  for (hipEvent_t& e : h->pipe_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  delete h;
}

const char* film_last_error(const film_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int film_set_option(film_t* h, const char* key, int64_t value) {
  if (!h || !key) return FILM_ERR_INVALID;
  for (const OptionRow& o : kOptions) {
    if (strcmp(key, o.key)) continue;
    if (o.refusal && (value < o.lo || value > o.hi)) return fail(h, FILM_ERR_INVALID, "%s", o.refusal);
    const int v = o.norm == BOOL ? value != 0 : o.norm == NONNEG ? (value > 0 ? (int)value : 0) : o.norm == LOW5 ? (int)(value & 31) : (int)value;
    if (o.family_refusal && v >= o.need_lo && v <= o.need_hi && !conv_family_built(o.family)) return fail(h, FILM_ERR_INVALID, o.family_refusal, v);
    if (!o.field) return h->finalized ? film_ensure_groups_(h, v) : FILM_OK;
    if (h->*o.field == v) return FILM_OK;   // (unchanged: the plans, last_plan and the autotuned tiles stay)
    if (o.drops_plans) drop_plans(h);
    h->*o.field = v;
    return FILM_OK;
  }
  return fail(h, FILM_ERR_NOTFOUND, "unknown option '%s'", key);
}

int film_plan_json(film_t* h, int B, int H, int W, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  Plan* P = nullptr;
  int rc = get_plan(h, B, H, W, false, &P);
  if (rc) return rc;
  return copy_out_string(h, plan_json(h, *P), buf, cap, needed);
}

int film_sequence_plan_json(film_t* h, int n_pairs, int tiles_per_frame, int H, int W, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  if (n_pairs < 1 || tiles_per_frame < 1) return fail(h, FILM_ERR_INVALID, "n_pairs and tiles_per_frame must be positive");
  if ((int64_t)n_pairs * tiles_per_frame >= (int64_t)1 << 30) return fail(h, FILM_ERR_INVALID, "batch too large (2*B*H*W must fit int32)");
  Plan* P = nullptr;
  int rc = get_plan(h, n_pairs * tiles_per_frame, H, W, false, &P, tiles_per_frame);
  if (rc) return rc;
  return copy_out_string(h, plan_json(h, *P), buf, cap, needed);
}

int film_profile_json(film_t* h, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  if (h->profile_json.empty()) return fail(h, FILM_ERR_STATE, "no profiled forward yet (film_set_option(\"profile\", 1))");
  return copy_out_string(h, h->profile_json, buf, cap, needed);
}

int film_forward(film_t* h, const float* x0, const float* x1, int B, int H, int W, float* out, int mem_kind, void* stream) {
  if (!h || !x0 || !x1 || !out) return fail(h, FILM_ERR_INVALID, "NULL argument");
  int rc = need_device(h, "film_forward");
  if (rc) return rc;
  if (mem_kind != FILM_MEM_HOST && mem_kind != FILM_MEM_DEVICE) return fail(h, FILM_ERR_INVALID, "bad mem_kind");
  if (B < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  int bmax = 1;
  rc = max_units(h, H, W, "frame", "tile the frame (Interpolator block_shape)", &bmax);
  if (rc) return rc;
  const size_t frame = (size_t)H * W * 3;
  int chunk = balanced_chunk(B, bmax);
  for (int b0 = 0; b0 < B;) {  // independent frame pairs: the batch splits with no change in results
    chunk = std::min(chunk, B - b0);
    rc = forward_chunk(h, x0 + b0 * frame, x1 + b0 * frame, chunk, H, W, out + b0 * frame, mem_kind, stream);
    if (halve_on_nomem(rc, &chunk)) continue;
    if (rc) return rc;
    b0 += chunk;
  }
  return FILM_OK;
}

int film_interpolate(film_t* h, const float* x0, const float* x1, int B, int H, int W, int align, int block_h,
                     int block_w, float* out, int mem_kind, void* stream) {
  if (!h || !x0 || !x1 || !out) return fail(h, FILM_ERR_INVALID, "NULL argument");
  int rc = need_device(h, "film_interpolate");
  if (rc) return rc;
  if (mem_kind != FILM_MEM_HOST && mem_kind != FILM_MEM_DEVICE) return fail(h, FILM_ERR_INVALID, "bad mem_kind");
  if (B < 1 || H < 1 || W < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  TileMapParams tp{};
  tp.B = B;
  rc = tile_geometry(h, H, W, block_h, block_w, align, &tp);
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  int tmax = 1;
  rc = max_units(h, tp.TH, tp.TW, "tile", "use a finer block_shape", &tmax);
  if (rc) return rc;
  const int ntiles = B * tp.bh * tp.bw;
  hipStream_t s = pick_stream(h, mem_kind, stream);
  const size_t nf = (size_t)B * H * W * 3;
  FrameStage st{h, s, mem_kind == FILM_MEM_HOST, out, nf};   // [x0 | x1 | out]
  rc = st.open(2 * nf);
  if (rc) return rc;
  // Host pipeline (round 6): one chunk on the direct two-lane executor - see interpolate_host_pipeline above.  It downloads the upper half of
  // the result before the lower tiles are done; with overlapped tiles that half depends on them, so they take the plain path
  if (st.host && h->opt_host_overlap && !(tp.ovy | tp.ovx) && !h->opt_profile && h->opt_graph == 2 && h->opt_lanes != 0 && ntiles <= tmax && h->stream2) {
    Plan* P = nullptr;
    rc = get_plan(h, ntiles, tp.TH, tp.TW, true, &P);
    if (rc == FILM_OK) return interpolate_host_pipeline(h, P, tp, x0, x1, out, (float*)h->stage, nf * sizeof(float), s);
    if (rc != FILM_ERR_NOMEM) return rc;   // (workspace did not fit: the chunked path below)
  }
  const float *d0 = nullptr, *d1 = nullptr;
  if ((rc = st.upload(x0, nf, &d0)) || (rc = st.upload(x1, nf, &d1))) return rc;
  int chunk = balanced_chunk(ntiles, tmax);
  for (int t0 = 0; t0 < ntiles;) {
    chunk = std::min(chunk, ntiles - t0);
    Plan* P = nullptr;
    rc = get_plan(h, chunk, tp.TH, tp.TW, true, &P);
    if (halve_on_nomem(rc, &chunk)) continue;
    if (rc == FILM_OK) rc = run_chunk(h, P, tp, {{d0, t0, chunk, 0}, {d1, t0, chunk, chunk}}, {{st.out, t0, chunk, 0}}, s);
    if (rc) return rc;
    t0 += chunk;
  }
  return st.finish();
}

int film_tiling_json(film_t* h, int H, int W, int align, int block_h, int block_w, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  if (H < 1 || W < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  TileMapParams tp{};
  int rc = tile_geometry(h, H, W, block_h, block_w, align, &tp);
  if (rc) return rc;
  std::ostringstream o;
  o << "{\"overlap_h\":" << tp.ovy << ",\"overlap_w\":" << tp.ovx << ",\"tile_h\":" << tp.eh << ",\"tile_w\":" << tp.ew
    << ",\"padded_h\":" << tp.TH << ",\"padded_w\":" << tp.TW << ",\"pad_y\":" << tp.oy << ",\"pad_x\":" << tp.ox << ",\"origins_y\":[";
  for (int i = 0; i < tp.bh; ++i) o << (i ? "," : "") << film_tile_origin(i, tp.ph, tp.ovy, tp.H, tp.eh);
  o << "],\"origins_x\":[";
  for (int j = 0; j < tp.bw; ++j) o << (j ? "," : "") << film_tile_origin(j, tp.pw, tp.ovx, tp.W, tp.ew);
  o << "]}";
  return copy_out_string(h, o.str(), buf, cap, needed);
}

int film_interpolate_sequence(film_t* h, const float* frames, int F, int H, int W, int align, int block_h, int block_w, float* out,
                              int mem_kind, void* stream) {
  // (the arguments are checked before the device: a plan-only handle reports them like a device handle does)
  if (!h || !frames || !out) return fail(h, FILM_ERR_INVALID, "NULL argument");
  if (mem_kind != FILM_MEM_HOST && mem_kind != FILM_MEM_DEVICE) return fail(h, FILM_ERR_INVALID, "bad mem_kind");
  if (F < 2) return fail(h, FILM_ERR_INVALID, "a sequence needs at least 2 frames, got %d", F);
  if (H < 1 || W < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  TileMapParams tp{};
  tp.B = 1;
  int rc = tile_geometry(h, H, W, block_h, block_w, align, &tp);
  if (rc == FILM_OK) rc = need_device(h, "film_interpolate_sequence");
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  int tmax = 1;
  rc = max_units(h, tp.TH, tp.TW, "tile", "use a finer block_shape", &tmax);
  if (rc) return rc;
  const int n = F - 1, T = tp.bh * tp.bw;
  int k = 1, nt = 1;
  sequence_chunk(n, T, tmax, &k, &nt);
  hipStream_t s = pick_stream(h, mem_kind, stream);
  const size_t frame = (size_t)H * W * 3;
  FrameStage st{h, s, mem_kind == FILM_MEM_HOST, out, n * frame};   // [F frames | F - 1 results]: plain upload, work, download
  const float* dfr = nullptr;
  if ((rc = st.open(F * frame)) || (rc = st.upload(frames, F * frame, &dfr))) return rc;
  for (int j0 = 0; j0 < n; j0 += k) {   // pairs j0 .. j0 + k of frames j0 .. j0 + k, a tile range at a time
    k = std::min(k, n - j0);
    for (int t0 = 0; t0 < T;) {
      const int nn = std::min(nt, T - t0);
      Plan* P = nullptr;
      rc = get_plan(h, k * nn, tp.TH, tp.TW, true, &P, nn);
      // workspace did not fit: smaller chunks - fewer pairs, then fewer tiles - and this block of pairs again from its first tile (a tile range
      // already done is recomputed into the same outputs, with the same bits; overlapped tiles: the ranges of a frame add up in tile order from
      // its first tile, so also after a halving)
      if (k * nn > 1 && (halve_on_nomem(rc, &k) || halve_on_nomem(rc, &nt))) { t0 = 0; continue; }
      if (rc) return rc;
      std::vector<Cut> cuts;
      std::vector<Join> joins;
      if (nn == T) {   // whole frames: frames j0 .. j0 + k are consecutive tiles of one frame batch, one launch each way
        cuts = {{dfr + j0 * frame, 0, (k + 1) * T, 0}};
        joins = {{st.out + j0 * frame, 0, k * T, 0}};
      } else {         // tiles [t0, t0 + nn) of each frame, frame-major
        for (int f = 0; f <= k; ++f) cuts.push_back({dfr + (j0 + f) * frame, t0, nn, (int64_t)f * nn});
        for (int j = 0; j < k; ++j) joins.push_back({st.out + (j0 + j) * frame, t0, nn, (int64_t)j * nn});
      }
      rc = run_chunk(h, P, tp, cuts, joins, s);
      if (rc) return rc;
      t0 += nn;
    }
  }
  return st.finish();
}

int film_get_tap(film_t* h, const char* name, float* dst, int64_t cap, int64_t dims[4]) {
  if (!h || !name) return FILM_ERR_INVALID;
  if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle has no device");
  Plan* P = h->last_plan;
  if (!P || !P->arena) return fail(h, FILM_ERR_STATE, "no forward has run yet");
  const int bi = P->find(name);
  if (bi < 0) return fail(h, FILM_ERR_NOTFOUND, "unknown tap '%s'", name);
  const Buffer& b = P->bufs[bi];
  for (const OpDesc& op : P->ops)   // a fused 1x1 head keeps this activation on chip: nothing ever writes the buffer
    if (op.kind == OP_CONV && op.pw_out.buf >= 0 && op.out.buf == bi)
      return fail(h, FILM_ERR_STATE, "tap '%s' is not materialised: the RGB head is fused into the layer that produces it "
                  "(film_set_option \"fuse\" without bit 16 keeps it)", name);
  if (dims) { dims[0] = b.N; dims[1] = b.H; dims[2] = b.W; dims[3] = b.C; }
  if (!dst) return FILM_OK;  // shape query
  if (cap < b.size()) return fail(h, FILM_ERR_INVALID, "capacity %lld < %lld floats", (long long)cap, (long long)b.size());
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipDeviceSynchronize());
  if (!b.planar) {
    HIPCHK(h, hipMemcpy(dst, P->arena + b.off, (size_t)b.size() * sizeof(float), hipMemcpyDeviceToHost));
    return FILM_OK;
  }
  // three pixel-major planes -> [N][H][W][C]
  std::vector<float> raw((size_t)b.size());
  HIPCHK(h, hipMemcpy(raw.data(), P->arena + b.off, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
  const int64_t npix = (int64_t)b.N * b.H * b.W;
  const int pc[3] = {b.planar, b.planar, b.C - 2 * b.planar};
  int64_t base = 0;
  int coff = 0;
  for (int part = 0; part < 3; ++part) {
    for (int64_t i = 0; i < npix; ++i) std::memcpy(dst + i * b.C + coff, raw.data() + base + i * pc[part], (size_t)pc[part] * sizeof(float));
    base += npix * pc[part];
    coff += pc[part];
  }
  return FILM_OK;
}

int film_debug_arena(film_t* h, int B, int H, int W, int tiles, int64_t offset, int64_t count, float* data, int write) {
  if (!h) return FILM_ERR_INVALID;
  if (!data || offset < 0 || count < 0) return fail(h, FILM_ERR_INVALID, "film_debug_arena: NULL data or a negative range");
  Plan* P = nullptr;
  int rc = debug_plan(h, B, H, W, tiles, &P);
  if (rc) return rc;
  if (offset > P->arena_floats || count > P->arena_floats - offset)
    return fail(h, FILM_ERR_INVALID, "film_debug_arena: floats %lld .. %lld leave the workspace of %lld floats", (long long)offset,
                (long long)(offset + count), (long long)P->arena_floats);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (count > 0) {
    if (write) HIPCHK(h, hipMemcpy(P->arena + offset, data, (size_t)count * sizeof(float), hipMemcpyHostToDevice));
    else HIPCHK(h, hipMemcpy(data, P->arena + offset, (size_t)count * sizeof(float), hipMemcpyDeviceToHost));
  }
  h->last_plan = P;
  return FILM_OK;
}

int film_debug_run_op(film_t* h, int B, int H, int W, int tiles, int index, int candidate, int* n_candidates) {
  if (!h) return FILM_ERR_INVALID;
  Plan* P = nullptr;
  int rc = debug_plan(h, B, H, W, tiles, &P);
  if (rc) return rc;
  if (index < 0 || (size_t)index >= P->ops.size())
    return fail(h, FILM_ERR_INVALID, "film_debug_run_op: op %d of a plan of %zu ops", index, P->ops.size());
  OpDesc op = P->ops[(size_t)index];
  std::vector<int> cands;
  if (op.kind == OP_CONV) cands = conv_candidates(op);
  if (n_candidates) *n_candidates = (int)cands.size();
  if (candidate < -1 || candidate >= (int)cands.size())   // (a non-conv op has no candidates: -1 only)
    return fail(h, FILM_ERR_INVALID, "film_debug_run_op: candidate %d of op %d ('%s'), which has %zu", candidate, index, op.tag.c_str(), cands.size());
  if (candidate >= 0) op.tile = cands[(size_t)candidate];
  HIPCHK(h, launch_op(op, P->arena, h->packed_dev, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->last_plan = P;
  return FILM_OK;
}

int film_debug_tile_map(film_t* h, int mode, int pix, void* frames_dev, float* tiles_dev, int B, int H, int W, int align, int block_h,
                        int block_w, int tile0, int ntiles, void* stream) {
  if (!h) return FILM_ERR_INVALID;
  if (!frames_dev || !tiles_dev) return fail(h, FILM_ERR_INVALID, "film_debug_tile_map: NULL argument");
  if (mode != 0 && mode != 1) return fail(h, FILM_ERR_INVALID, "film_debug_tile_map: bad mode %d: 0 (cut) or 1 (join)", mode);
  if (pix != FILM_PIX_F32 && pix != FILM_PIX_U8) return fail(h, FILM_ERR_INVALID, "bad pix: FILM_PIX_F32 (0) or FILM_PIX_U8 (1)");
  if (mode == 1 && pix == FILM_PIX_U8) return fail(h, FILM_ERR_INVALID, "film_debug_tile_map: a join writes float32 frames (FILM_PIX_U8 is for the cut only)");
  return debug_tile_map(h, "film_debug_tile_map", mode, pix, frames_dev, tiles_dev, B, H, W, align, block_h, block_w, tile0, ntiles, (hipStream_t)stream);
}

int film_debug_segment_copy(const int64_t* segs, int n, const float* src_dev, float* dst_dev, void* stream) {
  static_assert(sizeof(SegmentCopy) == 3 * sizeof(int64_t), "a row of `segs` is a SegmentCopy");
  const hipError_t e = film_launch_segment_copy(reinterpret_cast<const SegmentCopy*>(segs), n, src_dev, dst_dev, (hipStream_t)stream);   // (the refusals are the launcher's)
  return e == hipSuccess ? FILM_OK : e == hipErrorInvalidValue ? FILM_ERR_INVALID : FILM_ERR_HIP;
}

int film_debug_yuv_cut(film_t* h, int pix, void* frames_dev, float* tiles_dev, int B, int H, int W, int align, int block_h, int block_w,
                       int tile0, int ntiles, void* stream) {
  if (!h) return FILM_ERR_INVALID;
  if (!frames_dev || !tiles_dev) return fail(h, FILM_ERR_INVALID, "film_debug_yuv_cut: NULL argument");
  if (!pix_is_yuv(pix))
    return fail(h, FILM_ERR_INVALID, "film_debug_yuv_cut: bad pix layout %d: %s", pix_layout(pix), pix_layout_list(true).c_str());
  int rc = check_pix(h, pix, H, W);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(frames_dev) & 3) return fail(h, FILM_ERR_INVALID, "film_debug_yuv_cut: the frames of a Y'CbCr pix must be 4-byte aligned");
  return debug_tile_map(h, "film_debug_yuv_cut", 0, pix, frames_dev, tiles_dev, B, H, W, align, block_h, block_w, tile0, ntiles, (hipStream_t)stream);
}

}  // extern "C"

