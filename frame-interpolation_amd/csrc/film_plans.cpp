// film_plans.cpp -- the handle's plan cache: get_plan builds, tunes and keeps plans with their workspace arenas and evicts the least
// recently used; max_units says how many units one model invocation may take under the buffer and workspace limits.
#include "film_internal.h"

namespace film_internal {
namespace {
void free_plan(Plan* p) {
  for (auto& kv : p->orientations) free_plan(kv.second.get());
  if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
  if (p->graph) (void)hipGraphDestroy(p->graph);
  for (auto e : p->ev) (void)hipEventDestroy(e);
  for (auto e : p->lane_ev) if (e) (void)hipEventDestroy(e);
  if (p->arena && p->owns_arena) (void)hipFree(p->arena);
}

// Plan `index` leaves the cache with everything it holds on the device.  Work that may still run on it is the caller's to wait for.
void forget_plan(film_t* h, size_t index) {
  if (h->plans[index]->holds(h->last_plan)) h->last_plan = nullptr;
  free_plan(h->plans[index].get());
  h->plans.erase(h->plans.begin() + index);
}

constexpr int64_t kMaxBufferBytes = 0xFFF00000ll;
// One model invocation also keeps its workspace below this (a fifth of the HBM): 15 tiles of 960x576, one untiled 4K frame
constexpr int64_t kMaxArenaBytes = 64ll << 30;
// ... and below 60 % of the HBM this handle could get right now (free memory + what its own cached plans hold): other
// ranks' handles, torch's allocator or a smaller part may share the device.
int64_t arena_budget_bytes(film_t* h) {
  int64_t cap = kMaxArenaBytes;
  if (!h->plan_only) {
    size_t fr = 0, tot = 0;
    if (hipSetDevice(h->device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess) {
      int64_t held = 0;
      for (auto& p : h->plans) if (p->arena) held += p->arena_floats * (int64_t)sizeof(float);
      cap = std::min<int64_t>(cap, ((int64_t)fr + held) / 10 * 6);
    } else {
      (void)hipGetLastError();
    }
  }
  return std::max<int64_t>(cap, 1);
}

// test knobs: one tile shape for every F(4,3) / nested-Winograd / conv_fold4_kernel op it fits (same bits as any other, by construction)
void force_shapes(film_t* h, Plan* R) {
  const std::pair<ConvFamily, int> forced[] = {{FAM_W43, h->opt_w43_shape}, {FAM_W2D, h->opt_w2d_shape}, {FAM_FOLD4, h->opt_fold4_shape}};
  for (const auto& [fam, shape] : forced) {
    if (shape < 0) continue;
    for (OpDesc& op : R->ops) {
      if (op.kind != OP_CONV || op.family != fam) continue;
      const std::vector<int> cands = conv_candidates(op);
      const int want = conv_tile(fam, shape, true);
      if (std::find(cands.begin(), cands.end(), want) != cands.end()) op.tile = want;
    }
  }
}

}  // namespace

int plan_orientation(film_t* h, Plan* P0, int left, int right, bool extract, Plan** out) {
  if (P0->slots < 2) return fail(h, FILM_ERR_INVALID, "planner: not a stream plan");
  if (P0->left == left && P0->right == right && P0->extract == extract) { *out = P0; return FILM_OK; }
  const int key = Plan::orientation_key(left, right, extract);
  const auto it = P0->orientations.find(key);
  if (it != P0->orientations.end()) { *out = it->second.get(); return FILM_OK; }
  // first use: built over P0's buffers and checked against its layout
  std::unique_ptr<Plan> Q(new Plan);
  int rc = plan_build(h, Q.get(), P0->B, P0->H, P0->W, P0->tiles, P0->slots, left, right, extract);
  if (rc) return rc;
  bool alike = Q->arena_floats == P0->arena_floats && Q->bufs.size() == P0->bufs.size() && Q->n_extract == (extract ? P0->n_extract : 0);
  for (size_t i = 0; alike && i < Q->bufs.size(); ++i) alike = Q->bufs[i].name == P0->bufs[i].name && Q->bufs[i].off == P0->bufs[i].off && Q->bufs[i].floats == P0->bufs[i].floats;
  if (!alike) return fail(h, FILM_ERR_INVALID, "planner: the orientations of a stream plan lay out different workspaces");
  Q->id = P0->id;
  Q->arena = P0->arena;
  Q->owns_arena = false;
  // its conv shapes are the cache entry's, measured when the workspace was allocated: the choices are taken, nothing is timed - the
  // workspace holds the carried frames of a running stream
  if (Q->arena && h->opt_autotune && h->finalized && (rc = autotune_plan(h, Q.get(), false))) return rc;
  force_shapes(h, Q.get());
  *out = Q.get();
  P0->orientations[key] = std::move(Q);
  return FILM_OK;
}

void drop_plans(film_t* h) {
  if (!h->plan_only) { (void)hipSetDevice(h->device); (void)hipDeviceSynchronize(); }   // (forwards may still be running on them)
  while (!h->plans.empty()) forget_plan(h, h->plans.size() - 1);
}

// Plans are cached per (B, H, W, tiles, slots): tiles = 0 for pair plans, > 0 for sequence plans (Plan::tiles), slots >= 2 for the
// stream plan of `tiles` tiles over that many frame slots (Plan::right >= 0: all its orientations, one cache entry, one workspace) -
// the kinds never stand in for each other.  All count toward the three device plans kept alive.
int get_plan(film_t* h, int B, int H, int W, bool need_device, Plan** out, int tiles, int slots) {
  const bool stream = slots > 0;
  const auto same = [&](const Plan& p) { return p.B == B && p.H == H && p.W == W && p.tiles == tiles && p.slots == slots; };
  const int div = 1 << (h->cfg.pyramid_levels - 1);
  if (B < 1 || H < 1 || W < 1) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive");
  if (H % div || W % div)
    return fail(h, FILM_ERR_INVALID, "input height and width (%d x %d) must be divisible by %d = 2^(pyramid_levels-1); "
                "pad first (Interpolator align)", H, W, div);
  // tfa dense_image_warp needs a >= 2x2 grid at every warped level
  const int wl = std::max(h->cfg.pyramid_levels - 2, h->cfg.fusion_pyramid_levels - 1);
  if ((H >> wl) < 2 || (W >> wl) < 2)
    return fail(h, FILM_ERR_INVALID, "input %d x %d too small: warped pyramid level %d would be smaller than 2x2", H, W, wl);
  if ((int64_t)2 * B * H * W >= (int64_t)1 << 31) return fail(h, FILM_ERR_INVALID, "batch too large (2*B*H*W must fit int32)");
  if ((int64_t)slots * B * H * W >= (int64_t)1 << 31) return fail(h, FILM_ERR_INVALID, "batch too large (slots*B*H*W must fit int32: \"stream_times\")");
  for (auto& p : h->plans)
    if (same(*p) && (!need_device || p->arena)) { *out = p.get(); p->last_use = ++h->tick; return FILM_OK; }
  if (need_device)   // a description-only plan of this shape (film_plan_json, max_units) is superseded, not kept beside the new one
    for (size_t i = 0; i < h->plans.size(); ++i)
      if (same(*h->plans[i])) { forget_plan(h, i); break; }
  std::unique_ptr<Plan> P(new Plan);
  int rc = stream ? plan_build(h, P.get(), B, H, W, tiles, slots, 1, 0, true) : plan_build(h, P.get(), B, H, W, tiles);
  if (rc) return rc;
  P->id = ++h->plan_ids;
  if (need_device && slots > 2) {
    // the slots of "stream_times" > 1 grow the per-image buffers beyond what max_units has budgeted for a pair of frames
    const int64_t lim = limited_buffer_bytes(P.get()), bytes = P->arena_floats * (int64_t)sizeof(float);
    if (lim > kMaxBufferBytes || bytes > arena_budget_bytes(h))
      return fail(h, FILM_ERR_NOMEM, "stream_times = %d: the workspace of %d frame slots (%.1f MB, largest 32-bit addressed buffer %.1f MB) does not fit "
                  "(64 GiB / 60 %% of the free HBM of workspace, 4 GiB per buffer) - use a smaller \"stream_times\" or a finer block_shape",
                  slots - 1, slots, bytes * 1e-6, lim * 1e-6);
  }
  if (need_device) {
    // keep at most 3 device plans alive (workspaces are GBs at 1080p tiles)
    size_t alive = 0;
    for (auto& p : h->plans) alive += p->arena != nullptr;
    while (alive >= 3) {
      size_t victim = h->plans.size();
      for (size_t i = 0; i < h->plans.size(); ++i)
        if (h->plans[i]->arena && (victim == h->plans.size() || h->plans[i]->last_use < h->plans[victim]->last_use)) victim = i;
      if (victim == h->plans.size()) break;
      // a graph launch of the victim on the caller's stream may still be running (device-resident callers are
      // asynchronous): its graph, events and workspace must outlive it
      (void)hipSetDevice(h->device);
      (void)hipDeviceSynchronize();
      forget_plan(h, victim);
      --alive;
    }
    hipError_t e = hipMalloc(&P->arena, (size_t)P->arena_floats * sizeof(float));
    if (e != hipSuccess && alive > 0) {   // out of memory: give back the other plans' workspaces and try once more
      (void)hipGetLastError();
      (void)hipDeviceSynchronize();
      for (size_t i = h->plans.size(); i-- > 0;)
        if (h->plans[i]->arena) forget_plan(h, i);   // (last_plan is one of them: only a plan that ran is remembered)
      e = hipMalloc(&P->arena, (size_t)P->arena_floats * sizeof(float));
    }
    if (e != hipSuccess) {
      P->arena = nullptr;
      if (slots > 2)
        return fail(h, FILM_ERR_NOMEM, "workspace hipMalloc of %.1f MB (stream_times = %d: %d frame slots) failed: %s", P->arena_floats * 4e-6, slots - 1, slots,
                    hipGetErrorString(e));
      return fail(h, FILM_ERR_NOMEM, "workspace hipMalloc of %.1f MB failed: %s", P->arena_floats * 4e-6, hipGetErrorString(e));
    }
    HIPCHK(h, hipMemsetAsync(P->arena, 0, (size_t)P->arena_floats * sizeof(float), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->opt_autotune && h->finalized && (rc = autotune_plan(h, P.get()))) { free_plan(P.get()); return rc; }
  }
  force_shapes(h, P.get());
  // a stream plan: the orientation of the second push comes with it - no push of a running stream builds a plan, and film_stream_open
  // reports orientations that disagree about the layout; the deeper ones come on first use
  Plan* second = nullptr;
  if (stream && (rc = plan_orientation(h, P.get(), 0, 1, true, &second))) { free_plan(P.get()); return rc; }
  P->last_use = ++h->tick;
  *out = P.get();
  h->plans.push_back(std::move(P));
  return FILM_OK;
}

// Most H x W units (`what`: frame pairs / pair-tiles) one model invocation may take: what the plan of ONE unit says about the 4 GiB-per-buffer limit
// and the workspace budget, then option "max_batch".  A unit that is too large by itself is refused with `advice`.
int max_units(film_t* h, int H, int W, const char* what, const char* advice, int* units) {
  Plan* P1 = nullptr;
  int rc = get_plan(h, 1, H, W, false, &P1);
  if (rc) return rc;
  const int64_t lim = limited_buffer_bytes(P1);
  const int64_t arena = std::max<int64_t>(1, P1->arena_floats * (int64_t)sizeof(float));
  *units = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxBufferBytes / lim, arena_budget_bytes(h) / arena));
  if (lim > kMaxBufferBytes)
    return fail(h, FILM_ERR_INVALID, "a %d x %d %s needs a %.1f GB activation buffer in front of a kernel that addresses 4 GiB per "
                "buffer - %s", H, W, what, lim * 1e-9, advice);
  if (h->opt_max_batch) *units = std::min(*units, h->opt_max_batch);
  return FILM_OK;
}

}  // namespace film_internal
