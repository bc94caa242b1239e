// film_stream.cpp -- the frame streams of the C-ABI (film_stream_*; the contract: include/film_hip.h): the one open stream of a handle
// (FilmStream, film_internal.h), the schedule of a push, where the frames of a push live, the scene-cut and duplicate rules, and the JSON queries about
// the stream plan.  The stream plan and its orientations are the plan cache's (get_plan / plan_orientation, film_plans.cpp); tile geometry,
// the `pix` check and the stream choice are shared with the other entry points (film_engine.cpp).
#include "film_internal.h"

using namespace film_internal;

// The stream's device buffers go back and it is closed.  Work that may still use them is the caller's to wait for.
void film_internal::stream_free(film_t* h) {
  FilmStream& fs = h->fs;
  for (void* p : {fs.keep, fs.keep2, (void*)fs.result, (void*)fs.result8, (void*)fs.hist_dev, (void*)fs.diff_dev, (void*)fs.carry})
    if (p) (void)hipFree(p);
  if (fs.hist_pin) (void)hipHostFree(fs.hist_pin);
  if (fs.diff_pin) (void)hipHostFree(fs.diff_pin);
  fs = FilmStream{};
}

namespace {

// what of a TileMapParams tile_geometry decides: the same values cut the same tiles
bool same_geometry(const TileMapParams& a, const TileMapParams& b) {
  const int va[] = {a.H, a.W, a.bh, a.bw, a.ph, a.pw, a.TH, a.TW, a.oy, a.ox, a.ovy, a.ovx, a.eh, a.ew};
  const int vb[] = {b.H, b.W, b.bh, b.bw, b.ph, b.pw, b.TH, b.TW, b.oy, b.ox, b.ovy, b.ovx, b.eh, b.ew};
  return std::equal(std::begin(va), std::end(va), std::begin(vb));
}
// A frame of pixel type `pix` -> its tiles in slot `slot` of the plan's img0 (an 8-bit frame is dequantised by the cut itself)
hipError_t stream_cut(const void* frame, int pix, TileMapParams tp, const Plan* P, int slot, hipStream_t s) {
  tp.tile0 = 0; tp.ntiles = tp.bh * tp.bw;
  tp.src = (const float*)frame;
  tp.dst = P->at("img0") + (int64_t)slot * tp.ntiles * tp.TH * tp.TW * 3;
  return film_launch_cut_tiles(tp, pix, s);
}
// ... its tiles [tile0, tile0 + ntiles) to `dst` (a tile group: into the group plan's slot, or into the carry)
hipError_t stream_cut_range(const void* frame, int pix, TileMapParams tp, int tile0, int ntiles, float* dst, hipStream_t s) {
  tp.tile0 = tile0; tp.ntiles = ntiles;
  tp.src = (const float*)frame;
  tp.dst = dst;
  return film_launch_cut_tiles(tp, pix, s);
}

// The steps of ONE primed push of a "stream_times" = T stream whose input frame lands in slot `slot` (0 / 1; the frame before waits in the
// other one), in execution order - the reference's recursion (eval/util.py, _recursive_generator) depth first, restricted to C: the
// positions selected by `mask` (bit i - 1: position i; film_stream_select) and their ancestors.  A pair step runs the pair (frame in slot
// `left`, frame in slot `right`) - with `extract`, behind the extraction of the right frame, which no step has extracted before - and
// yields the frame at position `index` of the 2^T - 1 between the two inputs (1-based, temporal order), a depth-`depth` mid-frame; `deliver`:
// the position is selected, the frame goes to the caller.  feed >= 0: the result has a child in C and is cut, as float32, into slot
// `feed` = 1 + depth, where its children find it: the left child (left, feed) extracts it, the right child (feed, right) reads what the
// left one extracted.  When only the right child is in C, nobody has extracted the fed-back frame: a step that is no pair (`pair` = false)
// stands in front of the right child - the left child's orientation run to n_extract, like a first push; its `index` / `depth` are those
// of the frame it extracts.  An empty selection leaves one such step, for the pushed frame (position 2^T, depth 0).
struct StreamStep { int left, right, extract, index, depth, feed; bool deliver, pair; };
uint64_t full_mask(int T) { return ((uint64_t)1 << ((1 << T) - 1)) - 1; }
// the positions index - half + 1 .. index + half - 1: the subtree of the mid-frame at `index` whose parents are `half` positions away
uint64_t subtree_mask(int index, int half) { return (((uint64_t)1 << (2 * half - 1)) - 1) << (index - half); }
void stream_steps(int T, uint64_t mask, int left, int right, bool extract, int depth, int index, std::vector<StreamStep>* v) {
  const int half = depth < T ? 1 << (T - depth - 1) : 0;   // of the children (0: the deepest mids have none)
  const bool l = half && (mask & subtree_mask(index - half, half)), r = half && (mask & subtree_mask(index + half, half));
  const int feed = l || r ? 1 + depth : -1;
  v->push_back({left, right, extract ? 1 : 0, index, depth, feed, (mask >> (index - 1) & 1) != 0, true});
  if (l) stream_steps(T, mask, left, feed, true, depth + 1, index - half, v);
  else if (r) v->push_back({left, feed, 1, index, depth, -1, false, false});
  if (r) stream_steps(T, mask, feed, right, false, depth + 1, index + half, v);
}
std::vector<StreamStep> stream_schedule(int T, int slot, uint64_t mask) {
  std::vector<StreamStep> v;
  if (mask) stream_steps(T, mask, 1 - slot, slot, true, 1, 1 << (T - 1), &v);
  else v.push_back({1 - slot, slot, 1, 1 << T, 0, -1, false, false});
  return v;
}
std::vector<StreamStep> stream_schedule(int T, int slot) { return stream_schedule(T, slot, full_mask(T)); }

// Where the n = 2^times - 1 frames of a primed push live.  A host push downloads each frame as soon as it is there and waits once, so each
// has a place of its own on the device: a float32 stream's in fs.result; every other stream's - whose float32 frame is only joined,
// quantised and fed back - in fs.result8, behind ONE float32 frame in fs.result.  A device push writes straight into the caller's `mid`.
// film_stream_open sizes the two buffers from here, film_stream_push takes the places of frame k from here.
struct StreamFrames {
  size_t nv, fb, n;   // values of a float32 frame; bytes of a frame of the stream's pixel type; frames per push
  bool f32;
  StreamFrames(int pix, int H, int W, int times)
      : nv((size_t)H * W * 3), fb(frame_bytes(pix, H, W)), n(((size_t)1 << times) - 1), f32(pix_layout(pix) == FILM_PIX_F32) {}
  size_t result_bytes() const { return (f32 ? n : 1) * nv * sizeof(float); }   // of fs.result
  size_t result8_bytes() const { return f32 ? 0 : n * fb; }                    // of fs.result8 (0: the stream has none)
  // joined: the float32 frame the join writes; quant: the quantised frame (RGB bytes or a 4:2:0 frame), nullptr for a float32 stream;
  // host: where a host push downloads the frame to, fb bytes from `quant` or else `joined`, nullptr for a device push
  struct Place { float* joined; void *quant, *host; };
  Place place(const FilmStream& fs, void* mid, bool host, size_t k) const {   // of frame k (0-based, temporal order) of a push into `mid`
    void* out = (unsigned char*)mid + k * fb;   // (a float32 frame: fb = nv floats)
    if (f32) return {host ? fs.result + k * nv : (float*)out, nullptr, host ? out : nullptr};
    return {fs.result, host ? (void*)(fs.result8 + k * fb) : out, host ? out : nullptr};
  }
  // of a frame that is only fed back (film_stream_select: an ancestor that is not selected): joined in the stream's own fs.result - the
  // copies and cuts of a push are ordered on one stream - never quantised, downloaded or written to `mid`
  static Place fed_only(const FilmStream& fs) { return {fs.result, nullptr, nullptr}; }
};

// Whatever fails in a push behind this guard: the stream forgets its carried frame (as after film_stream_reset), and both streams are
// drained before the error goes back to the caller, who may then free or reuse `frame` / `mid`.
struct Unprime {
  film_t* h; hipStream_t s; bool armed;
  ~Unprime() { if (armed) { h->fs.primed = h->fs.hist_valid = false; (void)hipStreamSynchronize(h->stream2); (void)hipStreamSynchronize(s); } }
};
// option "profile": the pair runs of one push add up (the push sets the flag behind its first run), and the next call starts afresh
struct AppendProfile { film_t* h; ~AppendProfile() { h->profile_append = false; } };

// The plan that held the carried frame's pyramids was evicted or dropped since that frame was pushed (or the tiles changed): the frame is
// extracted again from the stream's own copy, into the slot where it was - the same ops on the same values, the same bits.
int stream_reextract(film_t* h, Plan* P0, const TileMapParams& tp, hipStream_t s) {
  const FilmStream& fs = h->fs;
  Plan* R = nullptr;
  int rc = plan_orientation(h, P0, 1 - fs.slot, fs.slot, true, &R);
  if (rc) return rc;
  HIPCHK(h, stream_cut(fs.keep, fs.pix, tp, R, fs.slot, s));
  return run_plan(h, R, s, R->n_extract);
}

// Option "scene_cut" = k > 0: the histogram of the frame in fs.keep, taken on `s`, downloaded and waited for; *cut = the rule's verdict
// against the carried histogram when the stream is primed and has one.  The new histogram becomes the carried one (valid once the push succeeds).
int stream_scene_cut(film_t* h, hipStream_t s, int k, bool* cut) {
  FilmStream& fs = h->fs;
  constexpr size_t bytes = FILM_HIST_BINS * sizeof(uint32_t);
  if (!fs.hist_dev) HIPCHK(h, hipMalloc((void**)&fs.hist_dev, bytes));
  if (!fs.hist_pin) HIPCHK(h, hipHostMalloc((void**)&fs.hist_pin, bytes, hipHostMallocDefault));
  HIPCHK(h, film_launch_frame_histogram(fs.keep, fs.H, fs.W, fs.pix, fs.hist_dev, s));
  HIPCHK(h, hipMemcpyAsync(fs.hist_pin, fs.hist_dev, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (fs.primed && fs.hist_valid) {
    int64_t D = 0;
    for (int i = 0; i < FILM_HIST_BINS; ++i) D += std::llabs((int64_t)fs.hist_pin[i] - (int64_t)fs.hist_prev[i]);
    fs.cut_distance = D;
    *cut = 1000 * D >= (int64_t)k * 2 * frame_samples(fs.pix, fs.H, fs.W);
  }
  fs.hist_valid = false;   // (until the push has succeeded)
  std::copy(fs.hist_pin, fs.hist_pin + FILM_HIST_BINS, fs.hist_prev);
  return FILM_OK;
}

// Option "dup_hi" = hi >= 0: `frame` goes to fs.keep2 on `s`; on a primed stream it is compared there with the carried frame in fs.keep
// (film_frame_diff's kernel), the 96 bytes are downloaded and waited for, and *dup = the rule's verdict (include/film_hip.h, "Duplicate
// frames").  The caller drops the push or swaps the two buffers.
int stream_duplicate(film_t* h, const void* frame, bool host, hipStream_t s, int hi, bool* dup) {
  FilmStream& fs = h->fs;
  const size_t fb = frame_bytes(fs.pix, fs.H, fs.W);
  constexpr size_t bytes = 12 * sizeof(uint64_t);
  if (!fs.keep2) HIPCHK(h, hipMalloc(&fs.keep2, (fb + 3) & ~(size_t)3));   // (whole 32-bit words, as fs.keep)
  if (!fs.diff_dev) HIPCHK(h, hipMalloc((void**)&fs.diff_dev, bytes));
  if (!fs.diff_pin) HIPCHK(h, hipHostMalloc((void**)&fs.diff_pin, bytes, hipHostMallocDefault));
  HIPCHK(h, hipMemcpyAsync(fs.keep2, frame, fb, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  if (!fs.primed) return FILM_OK;
  const int64_t m = pix_is_yuv10(fs.pix) ? 4 : 1;   // a value means the same on the 8- and 10-bit versions of one video
  HIPCHK(h, film_launch_frame_diff(fs.keep, fs.keep2, fs.H, fs.W, fs.pix, (int)(h->opt_dup_lo * m), fs.diff_dev, s));
  HIPCHK(h, hipMemcpyAsync(fs.diff_pin, fs.diff_dev, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  bool same = true;
  for (int p = 0; p < 3; ++p) {
    const uint64_t* o = fs.diff_pin + 4 * p;   // {total, max, over, blocks}
    for (int k = 0; k < 4; ++k) fs.dup_stats[4 * p + k] = (int64_t)o[k];
    same = same && (int64_t)o[1] <= hi * m && 1000 * (int64_t)o[2] <= (int64_t)h->opt_dup_frac * (int64_t)o[3];
  }
  *dup = same;
  return FILM_OK;
}

// The joined float32 frame of a result at p.joined -> its quantised frame (none for a float32 stream) -> the host (a host push: queued, not waited for)
int stream_quantise(film_t* h, const StreamFrames& fr, const StreamFrames::Place& p, hipStream_t s) {
  const FilmStream& fs = h->fs;
  if (p.quant && pix_is_yuv(fs.pix))
    HIPCHK(h, film_launch_rgb_to_yuv(p.joined, p.quant, fs.H, fs.W, fs.pix, s));
  else if (p.quant)
    HIPCHK(h, film_launch_to_uint8(p.joined, static_cast<uint8_t*>(p.quant), (int64_t)fr.nv, s));
  if (p.host) HIPCHK(h, hipMemcpyAsync(p.host, p.quant ? p.quant : (void*)p.joined, fr.fb, hipMemcpyDeviceToHost, s));
  return FILM_OK;
}

// One result of a push, the "out" tiles of the pair run Q, delivered to `p`: joined in float32 by the kernels of film_interpolate, then
// quantised by film_to_uint8's kernel for an 8-bit RGB stream, by film_to_yuv420's for a 4:2:0 stream (8-bit or 10-bit), then downloaded
// (a host push: queued, not waited for); feed >= 0: a result that has children is cut from the float32 frame - never from the quantised
// one - into slot `feed` by the float cut.
int stream_deliver(film_t* h, const Plan* Q, const TileMapParams& tp, const StreamFrames& fr, const StreamFrames::Place& p, int feed, hipStream_t s) {
  const FilmStream& fs = h->fs;
  TileMapParams j = tp;
  j.tile0 = 0; j.ntiles = tp.bh * tp.bw; j.src = Q->at("out"); j.dst = p.joined;
  HIPCHK(h, film_launch_join_tiles(j, s));
  int rc = stream_quantise(h, fr, p, s);
  if (rc) return rc;
  if (feed >= 0) HIPCHK(h, stream_cut(p.joined, FILM_PIX_F32, tp, Q, feed, s));
  return FILM_OK;
}

// ---- tile groups: a frame of more tiles than one invocation takes --------------------------------------------------------------------
// Such a stream runs its frame as G groups of n tiles through ONE stream plan of n tiles, group after group (the last group: the r <= n
// tiles that are left, on the same plan - its surplus images compute on what the group before left there, nobody reads them).  The carry,
// a device buffer of the stream's own, holds for every (group, frame slot) what a pair run reads of an extracted frame: before a group's
// run the slots it reads are copied from the carry into the plan, behind a run that extracted a frame that slot is copied out.  Every
// run is an ordinary run of an ordinary orientation, so the bits are those of the one-group stream.
//
// The carry buffers are the per-image buffers (slots * n images) that the ops of a pair run read and none of them writes - the image and
// feature pyramids.  Images are the outer dimension, so the images of one slot are one contiguous piece of each buffer, and the state of a
// (group, slot) is one segment per buffer.  The carry lays the segments out [group][slot][buffer], r * per_image floats each.
struct CarryLayout {
  std::vector<int> bufs;            // the carry buffers (indices into Plan::bufs), in plan order
  std::vector<int64_t> per_image;   // floats of one image of each ...
  int64_t image_floats = 0;         // ... and of all of them
  int img0 = -1;                    // where the cut's target, "img0", is among them
  int tiles = 0, n = 0, slots = 0;  // tiles of the frame, of a group (= of the plan), frame slots
  int groups() const { return (tiles + n - 1) / n; }
  int ntiles(int g) const { return std::min(n, tiles - g * n); }
  int64_t floats() const { return (int64_t)slots * tiles * image_floats; }
  int64_t carry_off(int g, int slot, size_t i) const {   // of buffer i of (group g, slot)
    int64_t o = ((int64_t)g * n * slots + (int64_t)slot * ntiles(g)) * image_floats;
    for (size_t k = 0; k < i; ++k) o += ntiles(g) * per_image[k];
    return o;
  }
  int64_t plan_off(const Plan* P, int slot, size_t i) const { return P->bufs[(size_t)bufs[i]].off + (int64_t)slot * n * per_image[i]; }
  // the segments of (group g, slot) - all of them, or only the img0 tiles a feed-cut left - appended to `out`: carry -> plan, or plan -> carry
  void segments(const Plan* P, int g, int slot, bool img0_only, bool restore, std::vector<SegmentCopy>* out) const {
    for (size_t i = 0; i < bufs.size(); ++i) {
      if (img0_only && (int)i != img0) continue;
      const int64_t c = carry_off(g, slot, i), p = plan_off(P, slot, i);
      out->push_back(restore ? SegmentCopy{c, p, ntiles(g) * per_image[i]} : SegmentCopy{p, c, ntiles(g) * per_image[i]});
    }
  }
};
int carry_layout(film_t* h, Plan* P0, int tiles, CarryLayout* L) {
  Plan* Q = nullptr;
  int rc = plan_orientation(h, P0, 1, 0, false, &Q);   // a pair run and nothing else
  if (rc) return rc;
  std::vector<char> rd(Q->bufs.size(), 0), wr(Q->bufs.size(), 0);
  std::vector<const View*> r, w;
  for (const OpDesc& op : Q->ops) {
    op_views(op, r, w);
    for (const View* v : r) rd[(size_t)v->buf] = 1;
    for (const View* v : w) wr[(size_t)v->buf] = 1;
  }
  *L = CarryLayout{};
  L->tiles = tiles; L->n = P0->tiles; L->slots = P0->slots;
  for (size_t b = 0; b < Q->bufs.size(); ++b) {
    const Buffer& B = Q->bufs[b];
    if (B.N != P0->slots * P0->tiles || !rd[b] || wr[b]) continue;
    if (B.planar) return fail(h, FILM_ERR_INVALID, "tile groups: the images of a slot of '%s' are no contiguous piece of it", B.name.c_str());
    if (B.name == "img0") L->img0 = (int)L->bufs.size();
    L->bufs.push_back((int)b);
    L->per_image.push_back((int64_t)B.H * B.W * B.C);
    L->image_floats += L->per_image.back();
  }
  if (L->img0 < 0) return fail(h, FILM_ERR_INVALID, "tile groups: a pair run does not read 'img0'");
  return FILM_OK;
}

// stream_schedule's steps, each expanded into the runs of its groups: outer = the steps, inner = the groups - a fed-back frame is the JOINED
// frame (cross-faded when "block_overlap_*" is set), which exists only when all groups of its step have run.  Per run:
//   restore  the slots copied whole from the carry into the plan in front of it: `left` of a pair run, and `right` when the run does not extract it
//   cut      where the frame it extracts comes from: CUT_KEEP - the pushed frame (slots 0 / 1), its tiles are cut from the stream's copy into the
//            plan; CUT_CARRY - a fed-back frame (slot 1 + depth), whose img0 tiles its parent's feed-cut left in the carry: they are restored;
//            one group (n >= tiles): CUT_PLAN - they are in the plan already
//   save     the slot copied whole from the plan into the carry behind it: `right` of a run that extracted it (-1: none)
//   join     a pair run's tiles go into the step's float32 frame; behind the `last` group's the frame is quantised and delivered, and one that
//            has children is cut, group by group, into the img0 segments of slot `feed` of the carry
// One group: the steps as they are, no restore, no save (what the one-group push does).
enum { CUT_NONE = 0, CUT_KEEP, CUT_CARRY, CUT_PLAN };
struct GroupStep {
  StreamStep t;
  int step, group, tile0, ntiles;
  int restore[2], nrestore;
  int cut, save;
  bool last;
};
std::vector<GroupStep> group_schedule(const std::vector<StreamStep>& steps, int tiles, int n) {
  const int G = (tiles + n - 1) / n;
  std::vector<GroupStep> v;
  for (size_t i = 0; i < steps.size(); ++i) {
    const StreamStep& t = steps[i];
    for (int g = 0; g < G; ++g) {
      GroupStep q{t, (int)i, g, g * n, std::min(n, tiles - g * n), {-1, -1}, 0, CUT_NONE, -1, g == G - 1};
      if (t.extract) q.cut = t.right < 2 ? CUT_KEEP : G > 1 ? CUT_CARRY : CUT_PLAN;
      if (G > 1) {
        if (t.pair) q.restore[q.nrestore++] = t.left;
        if (t.pair && !t.extract) q.restore[q.nrestore++] = t.right;
        if (t.extract) q.save = t.right;
      }
      v.push_back(q);
    }
  }
  return v;
}

// One launch per FILM_SEG_MAX segments (a restore of two slots of the published model: 28)
int copy_segments(film_t* h, const std::vector<SegmentCopy>& segs, const float* src, float* dst, hipStream_t s) {
  for (size_t i = 0; i < segs.size(); i += FILM_SEG_MAX)
    HIPCHK(h, film_launch_segment_copy(segs.data() + i, (int)std::min<size_t>(FILM_SEG_MAX, segs.size() - i), src, dst, s));
  return FILM_OK;
}

// The steps of a grouped push, run: `steps` is stream_schedule's list - of a primed push, or the one extraction-only step of a first push
// and of a re-extraction.  The runs of one call add up in the profile, as the pair runs of a one-group push do.
int run_group_steps(film_t* h, Plan* P0, const CarryLayout& L, const TileMapParams& tp, const std::vector<StreamStep>& steps, void* mid, bool host,
                    hipStream_t s, int* made) {
  FilmStream& fs = h->fs;
  AppendProfile append{h};
  const StreamFrames fr(fs.pix, fs.H, fs.W, fs.times);
  const int64_t tile_floats = (int64_t)tp.TH * tp.TW * 3;
  std::vector<SegmentCopy> segs;
  for (const GroupStep& g : group_schedule(steps, L.tiles, L.n)) {
    const StreamStep& t = g.t;
    Plan* Q = nullptr;
    int rc = plan_orientation(h, P0, t.left, t.right, t.extract != 0, &Q);
    if (rc) return rc;
    segs.clear();
    for (int i = 0; i < g.nrestore; ++i) L.segments(Q, g.group, g.restore[i], false, true, &segs);
    if (g.cut == CUT_CARRY) L.segments(Q, g.group, t.right, true, true, &segs);
    if ((rc = copy_segments(h, segs, fs.carry, Q->arena, s))) return rc;
    if (g.cut == CUT_KEEP)
      HIPCHK(h, stream_cut_range(fs.keep, fs.pix, tp, g.tile0, g.ntiles, Q->at("img0") + (int64_t)t.right * L.n * tile_floats, s));
    if ((rc = run_plan(h, Q, s, t.pair ? SIZE_MAX : Q->n_extract))) return rc;
    h->profile_append = true;
    if (g.save >= 0) {
      segs.clear();
      L.segments(Q, g.group, g.save, false, false, &segs);
      if ((rc = copy_segments(h, segs, Q->arena, fs.carry, s))) return rc;
    }
    if (!t.pair) continue;
    const size_t k = (size_t)__builtin_popcountll(fs.mask & (((uint64_t)1 << (t.index - 1)) - 1));   // selected positions before this one
    const StreamFrames::Place p = t.deliver ? fr.place(fs, mid, host, k) : StreamFrames::fed_only(fs);
    TileMapParams j = tp;   // (overlapped tiles: the joins of a frame add up in tile order on this one stream, group after group)
    j.tile0 = g.tile0; j.ntiles = g.ntiles; j.src = Q->at("out"); j.dst = p.joined;
    HIPCHK(h, film_launch_join_tiles(j, s));
    if (!g.last) continue;
    if ((rc = stream_quantise(h, fr, p, s))) return rc;
    // the step's frame is ONE buffer that the next step's joins reuse: a frame with children goes to the carry now, never from the quantised one
    for (int c = 0; t.feed >= 0 && c < L.groups(); ++c)
      HIPCHK(h, stream_cut_range(p.joined, FILM_PIX_F32, tp, c * L.n, L.ntiles(c), fs.carry + L.carry_off(c, t.feed, (size_t)L.img0), s));
    *made += t.deliver;
  }
  return FILM_OK;
}

// The carry of the frame geometry `tp`, allocated - or allocated again, when "block_overlap_*" grew the padded tile: such a change re-extracts
// every group anyway
int ensure_carry(film_t* h, const CarryLayout& L, const Plan* P0) {
  FilmStream& fs = h->fs;
  if (fs.carry && fs.carry_floats >= L.floats()) return FILM_OK;
  if (fs.carry) {
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipFree(fs.carry));
    fs.carry = nullptr; fs.carry_floats = 0;
  }
  const size_t bytes = (size_t)L.floats() * sizeof(float);   // (64-bit: 10 GB for a 4K frame's two slots)
  if (hipMalloc((void**)&fs.carry, bytes) != hipSuccess) {
    (void)hipGetLastError();
    fs.carry = nullptr;
    return fail(h, FILM_ERR_NOMEM, "hipMalloc of the stream's carry failed: workspace %lld bytes, carry %lld bytes (%d frame slots of %d tiles), %d tiles per group, %d groups",
                (long long)(P0->arena_floats * (int64_t)sizeof(float)), (long long)bytes, L.slots, L.tiles, L.n, L.groups());
  }
  fs.carry_floats = L.floats();
  return FILM_OK;
}

// film_stream_push of a stream of more than one group, behind the duplicate rule: the one-group push, step for step, over the carry.  The
// carry is the truth about the carried frame: a plan that was evicted and rebuilt needs no re-extraction; a changed tile geometry
// re-extracts every group from the stream's copy into the carry.
int push_groups(film_t* h, const void* frame, void* mid, int* produced, bool host, hipStream_t s, int dup_hi, Unprime* unprime) {
  FilmStream& fs = h->fs;
  TileMapParams tp{};
  tp.B = 1;
  int rc = tile_geometry(h, fs.H, fs.W, fs.block_h, fs.block_w, fs.align, &tp);   // ("block_overlap_*" as they are NOW)
  if (rc) return rc;
  Plan* P0 = nullptr;
  rc = get_plan(h, fs.group_tiles, tp.TH, tp.TW, true, &P0, fs.group_tiles, fs.times + 1);   // (n is the stream's: "max_batch" as it is now does not enter)
  if (rc) return rc;
  CarryLayout L;
  if ((rc = carry_layout(h, P0, tp.bh * tp.bw, &L)) || (rc = ensure_carry(h, L, P0))) return rc;
  int made = 0;
  if (fs.primed && !same_geometry(fs.geo, tp) && (rc = run_group_steps(h, P0, L, tp, stream_schedule(fs.times, fs.slot, 0), nullptr, host, s, &made))) return rc;
  if (dup_hi >= 0) std::swap(fs.keep, fs.keep2);   // (behind the re-extraction, which reads the carried frame's copy)
  else HIPCHK(h, hipMemcpyAsync(fs.keep, frame, frame_bytes(fs.pix, fs.H, fs.W), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  const int scene_k = h->opt_scene_cut;
  bool cut = false;
  if (scene_k > 0 && (rc = stream_scene_cut(h, s, scene_k, &cut))) return rc;
  const bool primed = fs.primed && !cut;
  const int slot = primed ? 1 - fs.slot : 0;
  // a first push is the push of an empty selection: the extraction of the pushed frame, group by group, into the carry
  if ((rc = run_group_steps(h, P0, L, tp, stream_schedule(fs.times, slot, primed ? fs.mask : 0), mid, host, s, &made))) return rc;
  if (host) HIPCHK(h, hipStreamSynchronize(s));
  *produced = made;
  fs.primed = true; fs.slot = slot; fs.plan_id = P0->id; fs.geo = tp;
  fs.hist_valid = scene_k > 0; fs.cut = cut ? 1 : 0;
  unprime->armed = false;
  return FILM_OK;
}

// film_stream_group_schedule_json: group_schedule's list, and in front of it the carry buffers of the plan the groups run on
std::string group_schedule_json(const Plan* P, const CarryLayout& L, int times, int slot, uint64_t mask) {
  static const char* const kCut[] = {"none", "keep", "carry", "plan"};
  const int G = L.groups();
  std::ostringstream o;
  o << "{\"times\":" << times << ",\"slot\":" << slot << ",\"slots\":" << times + 1 << ",\"mask\":" << mask << ",\"produced\":" << __builtin_popcountll(mask)
    << ",\"tiles\":" << L.tiles << ",\"group_tiles\":" << L.n << ",\"groups\":" << G << ",\"carry\":[";
  for (size_t i = 0; i < L.bufs.size(); ++i) o << (i ? "," : "") << "\"" << P->bufs[(size_t)L.bufs[i]].name << "\"";
  o << "],\"steps\":[";
  const std::vector<GroupStep> steps = group_schedule(stream_schedule(times, slot, mask), L.tiles, L.n);
  for (size_t i = 0; i < steps.size(); ++i) {
    const GroupStep& g = steps[i];
    const StreamStep& t = g.t;
    o << (i ? "," : "") << "{\"step\":" << g.step << ",\"group\":" << g.group << ",\"tile0\":" << g.tile0 << ",\"ntiles\":" << g.ntiles << ",\"left\":" << t.left
      << ",\"right\":" << t.right << ",\"extract\":" << t.extract << ",\"index\":" << t.index << ",\"depth\":" << t.depth << ",\"feed\":" << t.feed
      << ",\"deliver\":" << (t.deliver ? 1 : 0) << ",\"run\":\"" << (t.pair ? "pair" : "extract") << "\",\"restore\":[";
    for (int k = 0; k < g.nrestore; ++k) o << (k ? "," : "") << g.restore[k];
    o << "],\"cut\":\"" << kCut[g.cut] << "\",\"save\":" << g.save << ",\"join\":[";
    if (t.pair) o << g.tile0 << "," << g.ntiles;
    o << "],\"last\":" << (g.last ? 1 : 0) << ",\"feed_to\":\"" << (t.feed < 0 || !g.last ? "none" : G > 1 ? "carry" : "plan") << "\"}";
  }
  o << "]}";
  return o.str();
}

int check_schedule_query(film_t* h, int times, int slot) {
  if (times < 1 || times > kMaxStreamTimes) return fail(h, FILM_ERR_INVALID, "times must be 1 .. 6 (option \"stream_times\")");
  if (slot != 0 && slot != 1) return fail(h, FILM_ERR_INVALID, "slot must be 0 or 1 (the slot the pushed frame fills)");
  return FILM_OK;
}
int check_mask(film_t* h, int times, uint64_t mask) {
  if (mask & ~full_mask(times))
    return fail(h, FILM_ERR_INVALID, "mask has a bit at or above %d: a stream_times = %d push has positions 1 .. %d (bit i - 1: position i)",
                (1 << times) - 1, times, (1 << times) - 1);
  return FILM_OK;
}
// film_stream_schedule_json (mask == nullptr: the full push, the keys it always had) / film_stream_select_schedule_json
std::string schedule_json(int times, int slot, const uint64_t* mask) {
  const std::vector<StreamStep> steps = mask ? stream_schedule(times, slot, *mask) : stream_schedule(times, slot);
  const int produced = mask ? __builtin_popcountll(*mask) : (1 << times) - 1;
  std::ostringstream o;
  o << "{\"times\":" << times << ",\"slot\":" << slot << ",\"slots\":" << times + 1 << ",\"produced\":" << produced;
  if (mask) o << ",\"mask\":" << *mask;
  o << ",\"steps\":[";
  for (size_t i = 0; i < steps.size(); ++i) {
    const StreamStep& t = steps[i];
    o << (i ? "," : "") << "{\"left\":" << t.left << ",\"right\":" << t.right << ",\"extract\":" << t.extract << ",\"index\":" << t.index
      << ",\"depth\":" << t.depth << ",\"feed\":" << t.feed;
    if (mask) o << ",\"deliver\":" << (t.deliver ? 1 : 0) << ",\"run\":\"" << (t.pair ? "pair" : "extract") << "\"";
    o << "}";
  }
  o << "]}";
  return o.str();
}

}  // namespace

extern "C" {

int film_stream_plan_json(film_t* h, int tiles, int H, int W, int slot, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  if (tiles < 1) return fail(h, FILM_ERR_INVALID, "tiles must be positive");
  if (slot != 0 && slot != 1) return fail(h, FILM_ERR_INVALID, "slot must be 0 or 1 (the half of the frame buffers the pushed frame fills)");
  if (tiles >= 1 << 30) return fail(h, FILM_ERR_INVALID, "batch too large (2*B*H*W must fit int32)");
  Plan *P = nullptr, *Q = nullptr;
  int rc = get_plan(h, tiles, H, W, false, &P, tiles, 2);
  if (rc == FILM_OK) rc = plan_orientation(h, P, 1 - slot, slot, true, &Q);
  if (rc) return rc;
  return copy_out_string(h, plan_json(h, *Q), buf, cap, needed);
}

int film_stream_pair_plan_json(film_t* h, int tiles, int H, int W, int times, int left, int right, int extract, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  if (tiles < 1) return fail(h, FILM_ERR_INVALID, "tiles must be positive");
  if (times < 1 || times > kMaxStreamTimes) return fail(h, FILM_ERR_INVALID, "times must be 1 .. 6 (option \"stream_times\")");
  if (left < 0 || right < 0 || left > times || right > times || left == right)
    return fail(h, FILM_ERR_INVALID, "left and right must be two different slots of 0 .. %d (times + 1 frame slots)", times);
  if (tiles >= 1 << 30) return fail(h, FILM_ERR_INVALID, "batch too large (2*B*H*W must fit int32)");
  Plan *P = nullptr, *Q = nullptr;
  int rc = get_plan(h, tiles, H, W, false, &P, tiles, times + 1);
  if (rc == FILM_OK) rc = plan_orientation(h, P, left, right, extract != 0, &Q);
  if (rc) return rc;
  return copy_out_string(h, plan_json(h, *Q, true), buf, cap, needed);
}

int film_stream_schedule_json(film_t* h, int times, int slot, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  int rc = check_schedule_query(h, times, slot);
  if (rc) return rc;
  return copy_out_string(h, schedule_json(times, slot, nullptr), buf, cap, needed);
}

int film_stream_select_schedule_json(film_t* h, int times, int slot, uint64_t mask, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  int rc = check_schedule_query(h, times, slot);
  if (rc == FILM_OK) rc = check_mask(h, times, mask);
  if (rc) return rc;
  return copy_out_string(h, schedule_json(times, slot, &mask), buf, cap, needed);
}

int film_stream_group_schedule_json(film_t* h, int tiles, int H, int W, int times, int slot, uint64_t mask, int group_tiles, char* buf, int64_t cap,
                                    int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  if (tiles < 1 || group_tiles < 1) return fail(h, FILM_ERR_INVALID, "tiles and group_tiles must be positive");
  int rc = check_schedule_query(h, times, slot);
  if (rc == FILM_OK) rc = check_mask(h, times, mask);
  if (rc) return rc;
  const int n = std::min(tiles, group_tiles);
  if (n >= 1 << 30) return fail(h, FILM_ERR_INVALID, "batch too large (2*B*H*W must fit int32)");
  Plan* P = nullptr;
  CarryLayout L;
  if ((rc = get_plan(h, n, H, W, false, &P, n, times + 1)) || (rc = carry_layout(h, P, tiles, &L))) return rc;
  return copy_out_string(h, group_schedule_json(P, L, times, slot, mask), buf, cap, needed);
}

int film_stream_layout_json(film_t* h, char* buf, int64_t cap, int64_t* needed) {
  if (!h) return FILM_ERR_INVALID;
  const FilmStream& fs = h->fs;
  if (!fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  TileMapParams tp{};
  tp.B = 1;
  int rc = tile_geometry(h, fs.H, fs.W, fs.block_h, fs.block_w, fs.align, &tp);   // ("block_overlap_*" as they are NOW)
  if (rc) return rc;
  Plan* P = nullptr;
  CarryLayout L;
  const bool grouped = fs.groups > 1;   // (one group: no carry, nothing to derive)
  if ((rc = get_plan(h, fs.group_tiles, tp.TH, tp.TW, false, &P, fs.group_tiles, fs.times + 1)) || (grouped && (rc = carry_layout(h, P, tp.bh * tp.bw, &L)))) return rc;
  std::ostringstream o;
  o << "{\"tiles\":" << tp.bh * tp.bw << ",\"groups\":" << fs.groups << ",\"group_tiles\":" << fs.group_tiles << ",\"slots\":" << fs.times + 1
    << ",\"tile_h\":" << tp.TH << ",\"tile_w\":" << tp.TW << ",\"workspace_bytes\":" << P->arena_floats * (int64_t)sizeof(float) << ",\"workspace_resident\":" << (P->arena ? 1 : 0)
    << ",\"carry_bytes\":" << (grouped ? L.floats() * (int64_t)sizeof(float) : 0) << ",\"carry\":[";
  for (size_t i = 0; grouped && i < L.bufs.size(); ++i) o << (i ? "," : "") << "\"" << P->bufs[(size_t)L.bufs[i]].name << "\"";
  o << "],\"states\":[";
  for (int g = 0; grouped && g < fs.groups; ++g)
    for (int sl = 0; sl <= fs.times; ++sl) {
      o << (g || sl ? "," : "") << "{\"group\":" << g << ",\"slot\":" << sl << ",\"tile0\":" << g * L.n << ",\"ntiles\":" << L.ntiles(g) << ",\"segments\":[";
      for (size_t i = 0; i < L.bufs.size(); ++i)
        o << (i ? "," : "") << "{\"buf\":\"" << P->bufs[(size_t)L.bufs[i]].name << "\",\"plan_off\":" << L.plan_off(P, sl, i) << ",\"carry_off\":" << L.carry_off(g, sl, i)
          << ",\"floats\":" << L.ntiles(g) * L.per_image[i] << "}";
      o << "]}";
    }
  o << "]}";
  return copy_out_string(h, o.str(), buf, cap, needed);
}

int film_stream_select(film_t* h, uint64_t mask) {
  if (!h) return FILM_ERR_INVALID;
  if (!h->fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  int rc = check_mask(h, h->fs.times, mask);
  if (rc) return rc;
  h->fs.mask = mask;
  return FILM_OK;
}

int film_stream_open(film_t* h, int H, int W, int align, int block_h, int block_w, int pix) {
  if (!h) return FILM_ERR_INVALID;
  if (h->fs.open) return fail(h, FILM_ERR_STATE, "a stream is already open on this handle (one per handle: close it, or create another handle)");
  int rc = check_pix(h, pix, H, W);
  if (rc) return rc;
  if (H < 1 || W < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  TileMapParams tp{};
  tp.B = 1;
  rc = tile_geometry(h, H, W, block_h, block_w, align, &tp);
  if (rc == FILM_OK) rc = need_device(h, "film_stream_open");
  if (rc) return rc;
  HIPCHK(h, hipSetDevice(h->device));
  int tmax = 1;
  rc = max_units(h, tp.TH, tp.TW, "tile", "use a finer block_shape", &tmax);
  if (rc) return rc;
  const int T = tp.bh * tp.bw;
  const int times = h->opt_stream_times;   // fixed for this stream's life
  // The whole frame in one invocation where that fits (one group: the stream it always was); else tile groups of n tiles through the plan
  // of n tiles, n halved while its workspace does not fit.  Only a single tile that is too large is refused.
  int n = balanced_chunk(T, tmax);
  Plan* P = nullptr;
  do rc = get_plan(h, n, tp.TH, tp.TW, true, &P, n, times + 1);   // (built and tuned now; FILM_ERR_NOMEM when the workspace does not fit)
  while (halve_on_nomem(rc, &n));
  if (rc) return rc;
  FilmStream& fs = h->fs;
  const StreamFrames fr(pix, H, W, times);
  hipError_t e = hipMalloc(&fs.keep, (fr.fb + 3) & ~(size_t)3);   // (whole 32-bit words: the 8-bit cuts read aligned words)
  if (e == hipSuccess) e = hipMalloc((void**)&fs.result, fr.result_bytes());
  if (e == hipSuccess && fr.result8_bytes()) e = hipMalloc((void**)&fs.result8, fr.result8_bytes());
  if (e != hipSuccess) {
    (void)hipGetLastError();
    stream_free(h);
    return fail(h, FILM_ERR_NOMEM, "hipMalloc of the stream's frame buffers (%.1f MB, stream_times = %d) failed",
                (fr.fb + fr.result_bytes() + fr.result8_bytes()) * 1e-6, times);
  }
  fs.times = times;
  fs.group_tiles = n; fs.groups = (T + n - 1) / n;   // fixed for this stream's life, whatever "max_batch" says later
  if (fs.groups > 1) {
    CarryLayout L;
    if ((rc = carry_layout(h, P, T, &L)) || (rc = ensure_carry(h, L, P))) { stream_free(h); return rc; }
  }
  fs.open = true;
  fs.mask = full_mask(times);
  fs.H = H; fs.W = W; fs.align = align; fs.block_h = block_h; fs.block_w = block_w; fs.pix = pix;
  return FILM_OK;
}

int film_stream_reset(film_t* h) {
  if (!h) return FILM_ERR_INVALID;
  if (!h->fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  h->fs.primed = false;
  h->fs.hist_valid = false;
  return FILM_OK;
}

int film_stream_cut_info(film_t* h, int64_t* distance, int64_t* samples, int* cut) {
  if (!h) return FILM_ERR_INVALID;
  const FilmStream& fs = h->fs;
  if (!fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  if (distance) *distance = fs.cut_distance;
  if (samples) *samples = frame_samples(fs.pix, fs.H, fs.W);
  if (cut) *cut = fs.cut;
  return FILM_OK;
}

int film_stream_dup_info(film_t* h, int64_t* stats, int* dup) {
  if (!h) return FILM_ERR_INVALID;
  const FilmStream& fs = h->fs;
  if (!fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  if (stats) std::copy(fs.dup_stats, fs.dup_stats + 12, stats);
  if (dup) *dup = fs.dup;
  return FILM_OK;
}

int film_stream_close(film_t* h) {
  if (!h) return FILM_ERR_INVALID;
  if (!h->fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();   // (device-resident pushes are asynchronous: what they read must outlive them)
  stream_free(h);
  return FILM_OK;
}

// The order of the device work of a push - (option "dup_hi": copy beside the carried frame, compare, download, wait; a duplicate ends here) keep-copy; histogram, download, wait (option "scene_cut"); cut; per step of the schedule: run,
// join, quantise, download, feed-cut; one wait for a host push - is what lets a host push download a frame beside the next pair run, and
// what makes it hold for pageable memory, whose copies block the calling thread.
int film_stream_push(film_t* h, const void* frame, void* mid, int* produced, int mem_kind, void* stream) {
  if (!h) return FILM_ERR_INVALID;
  FilmStream& fs = h->fs;
  if (!fs.open) return fail(h, FILM_ERR_STATE, "no open stream (film_stream_open)");
  hipStream_t s = pick_stream(h, mem_kind == FILM_MEM_DEVICE ? FILM_MEM_DEVICE : FILM_MEM_HOST, stream);
  Unprime unprime{h, s, true};   // (whatever fails from here on)
  if (produced) *produced = 0;
  fs.cut_distance = -1; fs.cut = 0;
  if (!frame || !produced || (fs.primed && fs.mask && !mid)) return fail(h, FILM_ERR_INVALID, "NULL argument");
  if (mem_kind != FILM_MEM_HOST && mem_kind != FILM_MEM_DEVICE) return fail(h, FILM_ERR_INVALID, "bad mem_kind");
  HIPCHK(h, hipSetDevice(h->device));
  const bool host = mem_kind == FILM_MEM_HOST;
  // option "dup_hi": duplicates are decided first - a dropped push leaves the stream as it was (the plan and the carried histogram included)
  const int dup_hi = h->opt_dup_hi;
  std::fill(fs.dup_stats, fs.dup_stats + 12, (int64_t)-1); fs.dup = 0;
  int rc = FILM_OK;
  if (dup_hi >= 0) {
    bool dup = false;
    if ((rc = stream_duplicate(h, frame, host, s, dup_hi, &dup))) return rc;
    if (dup) {
      fs.dup = 1;
      unprime.armed = false;
      return FILM_OK;
    }
  }
  if (fs.groups > 1) return push_groups(h, frame, mid, produced, host, s, dup_hi, &unprime);
  TileMapParams tp{};
  tp.B = 1;
  rc = tile_geometry(h, fs.H, fs.W, fs.block_h, fs.block_w, fs.align, &tp);   // ("block_overlap_*" as they are NOW)
  if (rc) return rc;
  const int T = tp.bh * tp.bw;
  Plan* P0 = nullptr;
  rc = get_plan(h, T, tp.TH, tp.TW, true, &P0, T, fs.times + 1);
  if (rc) return rc;
  if (fs.primed && (fs.plan_id != P0->id || !same_geometry(fs.geo, tp)) && (rc = stream_reextract(h, P0, tp, s))) return rc;
  if (dup_hi >= 0) std::swap(fs.keep, fs.keep2);   // (behind the re-extraction, which reads the carried frame's copy)
  else HIPCHK(h, hipMemcpyAsync(fs.keep, frame, frame_bytes(fs.pix, fs.H, fs.W), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  // option "scene_cut": a cut is film_stream_reset followed by this push - the frame starts a new scene in slot 0, extraction only
  const int scene_k = h->opt_scene_cut;
  bool cut = false;
  if (scene_k > 0 && (rc = stream_scene_cut(h, s, scene_k, &cut))) return rc;
  const bool primed = fs.primed && !cut;
  const int slot = primed ? 1 - fs.slot : 0;
  Plan* P = nullptr;
  if ((rc = plan_orientation(h, P0, 1 - slot, slot, true, &P))) return rc;
  HIPCHK(h, stream_cut(fs.keep, fs.pix, tp, P, slot, s));
  int made = 0;
  if (!primed) {
    if ((rc = run_plan(h, P, s, P->n_extract))) return rc;
  } else {
    // one pair run per member of the selection and its ancestors, in the order of stream_schedule (times = 1: the one pair of the two
    // inputs); the selected frames are packed into `mid` in temporal order
    AppendProfile append{h};
    const StreamFrames fr(fs.pix, fs.H, fs.W, fs.times);
    for (const StreamStep& t : stream_schedule(fs.times, slot, fs.mask)) {
      Plan* Q = nullptr;
      if ((rc = plan_orientation(h, P0, t.left, t.right, t.extract != 0, &Q)) || (rc = run_plan(h, Q, s, t.pair ? SIZE_MAX : Q->n_extract))) return rc;
      h->profile_append = true;
      if (!t.pair) continue;
      const size_t k = (size_t)__builtin_popcountll(fs.mask & (((uint64_t)1 << (t.index - 1)) - 1));   // selected positions before this one
      if ((rc = stream_deliver(h, Q, tp, fr, t.deliver ? fr.place(fs, mid, host, k) : StreamFrames::fed_only(fs), t.feed, s))) return rc;
      made += t.deliver;
    }
  }
  if (host) HIPCHK(h, hipStreamSynchronize(s));
  *produced = made;
  fs.primed = true; fs.slot = slot; fs.plan_id = P0->id; fs.geo = tp;
  fs.hist_valid = scene_k > 0; fs.cut = cut ? 1 : 0;
  unprime.armed = false;
  return FILM_OK;
}

}  // extern "C"
