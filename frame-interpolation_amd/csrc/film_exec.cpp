// film_exec.cpp -- the executor: one planned op as a kernel launch (launch_op), a plan's ops on two lanes (issue_lanes) and run_plan, which
// runs a plan eagerly, as a hipGraph replay or op by op with events (option "profile": the text of film_profile_json).
#include "film_internal.h"

namespace film_internal {
namespace {
inline const float* cptr(const float* base, const View& v) { return base + v.off; }
inline float* mptr(float* base, const View& v) { return base + v.off; }
}  // namespace

hipError_t launch_op(const OpDesc& op, float* arena, const float* wts, hipStream_t s) {
  switch (op.kind) {
    case OP_CONV: {
      ConvParams p{};
      p.nseg = op.nseg;
      for (int i = 0; i < op.nseg; ++i) {
        p.seg[i].ptr = cptr(arena, op.seg[i].v);
        p.seg[i].stride = op.seg[i].v.stride;
        p.seg[i].C = op.seg[i].v.C;
        p.seg[i].boff = op.seg[i].boff; p.seg[i].bmod = op.seg[i].bmod; p.seg[i].up = op.seg[i].up;
      }
      p.ksize = op.ksize;
      p.w = wts + op.*kConvFamily[op.family].weights;
      p.bias = wts + op.b_off;
      p.out = mptr(arena, op.out); p.ostride = op.out.stride;
      p.NB = op.NB; p.H = op.H; p.W = op.W; p.Cout = op.Cout; p.Ctot = op.Ctot; p.leaky = op.leaky;
      p.M = op.NB * op.H * op.W;
      p.fold = op.fold; p.py = op.py; p.px = op.px; p.ftaps = op.ftaps;
      p.ksplit = op.ksplit; p.part = op.ksplit > 1 ? arena + op.part_off : nullptr;
      if (op.out2.buf >= 0) { p.pool_out = mptr(arena, op.out2); p.pool_ostride = op.out2.stride; }
      if (op.pw_out.buf >= 0) {
        p.pw_w = wts + op.w2_off; p.pw_bias = wts + op.b2_off; p.pw_out = mptr(arena, op.pw_out); p.pw_ostride = op.pw_out.stride; p.pw_cout = op.pw_cout;
      }
      for (int q = 0; q < 4; ++q) { p.tdy[q] = (signed char)op.tdy[q]; p.tdx[q] = (signed char)op.tdx[q]; p.fold_woff[q] = op.fold_woff[q]; }
      return film_launch_conv(p, op.tile, s);
    }
    case OP_FLOW_HEAD: {
      FlowHeadParams p{};
      p.in = cptr(arena, op.in); p.istride = op.in.stride; p.Cin = op.Ctot;
      p.w3 = wts + op.w_off; p.b3 = wts + op.b_off; p.w4 = wts + op.w2_off; p.b4 = wts + op.b2_off;
      p.out = mptr(arena, op.out); p.M = (int)op.n;
      if (op.out2.buf >= 0) { p.add = cptr(arena, op.in2); p.sum = mptr(arena, op.out2); }
      return film_launch_flow_head(p, s);
    }
    case OP_CONV_PW: {
      ConvPwParams p{};
      p.in = cptr(arena, op.in); p.istride = op.in.stride; p.Cin = op.Ctot;
      p.w = wts + op.w_off; p.bias = wts + op.b_off;
      p.out = mptr(arena, op.out); p.ostride = op.out.stride; p.Cout = op.Cout; p.leaky = op.leaky;
      p.M = (int)op.n;
      if (op.out2.buf >= 0) { p.add = cptr(arena, op.in2); p.sum = mptr(arena, op.out2); }
      return film_launch_conv_pw(p, s);
    }
    case OP_POOL: {
      PoolParams p{};
      p.in = cptr(arena, op.in); p.istride = op.in.stride; p.out = mptr(arena, op.out); p.ostride = op.out.stride;
      p.C = op.in.C; p.NB = op.NB; p.H = op.H; p.W = op.W;
      return film_launch_pool(p, s);
    }
    case OP_FLOW_UP: {
      FlowUpParams p{};
      p.in = cptr(arena, op.in); p.out = mptr(arena, op.out); p.NB = op.NB; p.h = op.H; p.w = op.W;
      return film_launch_flow_up(p, s);
    }
    case OP_FLOW_ADD: {
      FlowAddParams p{};
      p.a = cptr(arena, op.in); p.b = cptr(arena, op.in2); p.out = mptr(arena, op.out); p.n = op.n;
      return film_launch_flow_add(p, s);
    }
    case OP_WARP: {
      WarpParams p{};
      p.src = cptr(arena, op.in); p.sstride = op.in.stride; p.C = op.in.C;
      p.flow = op.in2.buf >= 0 ? cptr(arena, op.in2) : nullptr; p.fscale = op.fscale;
      p.dst = mptr(arena, op.out); p.dstride = op.out.stride;
      p.NB = op.NB; p.H = op.H; p.W = op.W;
      p.src_brot = op.src_brot; p.flow_brot = op.flow_brot; p.misc_nb = op.misc_nb;
      if (op.in3.buf >= 0) { p.coarse = cptr(arena, op.in3); p.flow_out = mptr(arena, op.out2); }
      if (op.img_out.buf >= 0) {   // misc16: both images (img_in = [2 NB] images), both flows
        p.src3 = cptr(arena, op.img_in); p.s3stride = op.img_in.stride;
        p.src3b = p.src3 + (int64_t)(op.misc_nb > 0 ? op.misc_nb : op.NB) * op.H * op.W * op.img_in.stride;
        p.dst3 = mptr(arena, op.img_out); p.d3stride = op.img_out.stride;
        p.pack_b = cptr(arena, op.pack_b); p.pack_f = cptr(arena, op.pack_f);
      }
      return film_launch_warp(p, s);
    }
    case OP_PACK_FLOW: {
      PackFlowParams p{};
      p.bflow = cptr(arena, op.in); p.fflow = cptr(arena, op.in2);
      p.dst = mptr(arena, op.out); p.dstride = op.out.stride; p.npix = op.n;
      return film_launch_pack_flow(p, s);
    }
  }
  return hipErrorInvalidValue;
}

// ---- batch parts of an op (the overlapped host path of film_interpolate) --------------------------------------------------------
// A convolution whose input is ONE segment without a batch remap computes every image of its batch independently: images
// [part * NB / nparts, (part + 1) * NB / nparts) as a launch of their own give the same bits (the kernel family and the tile are the op's).
bool batch_splittable(const OpDesc& op, int nparts) {
  return op.kind == OP_CONV && op.nseg == 1 && op.seg[0].bmod == 0 && op.seg[0].boff == 0 && op.seg[0].up == 0 && op.ksplit <= 1 && op.fold == 0 &&
         op.NB >= nparts && op.NB % nparts == 0 && (op.out2.buf < 0 || (!(op.H & 1) && !(op.W & 1)));
}
OpDesc batch_part(const OpDesc& op, int part, int nparts) {
  OpDesc q = op;
  q.NB = op.NB / nparts;
  const int64_t px = (int64_t)part * q.NB * op.H * op.W;
  q.seg[0].v.off += px * op.seg[0].v.stride;
  q.out.off += px * op.out.stride;
  if (op.out2.buf >= 0) q.out2.off += (int64_t)part * q.NB * (op.H / 2) * (op.W / 2) * op.out2.stride;
  if (op.pw_out.buf >= 0) q.pw_out.off += px * op.pw_out.stride;
  return q;
}

// The plan's ops on two lanes: lane 0 on `main`, lane 1 (small subtrees, coarse flow levels, the t = 0.5 warps) on the handle's side
// stream, forked from and joined to `main`; cross-lane ordering = the events found by Planner::analyze_lanes (each op is waited for
// at most once by the other lane - see there for why that matters to a graph replay).  Called inside a stream capture (graph = 1:
// the events become graph edges) or directly (graph = 2: real events; one set per plan, re-recorded every forward - a wait refers
// to the record that precedes it in program order, and everything of forward n + 1 is ordered behind forward n's join on `main`).
hipError_t issue_lanes(film_t* h, Plan* P, hipStream_t main, bool capturing, const LanePipe* lp) {
  const size_t nops = P->ops.size();
  if (P->lane_ev.size() < nops + 2) P->lane_ev.resize(nops + 2, nullptr);
  hipError_t ev_err = hipSuccess;
  auto event_of = [&](size_t i) -> hipEvent_t {
    if (!P->lane_ev[i]) {
      hipError_t e = hipEventCreateWithFlags(&P->lane_ev[i], hipEventDisableTiming);
      if (e != hipSuccess) { ev_err = e; P->lane_ev[i] = nullptr; }
    }
    return P->lane_ev[i];
  };
  const bool two_lanes = h->opt_lanes != 0;
  hipError_t le = hipSuccess;
  if (two_lanes) {
    le = hipEventRecord(event_of(nops), main);
    if (le == hipSuccess) le = hipStreamWaitEvent(h->stream2, event_of(nops), 0);
  }
  for (size_t i = 0; i < nops && le == hipSuccess; ++i) {
    const OpDesc& op = P->ops[i];
    const int lane = (two_lanes && op.lane == 1) ? 1 : 0;
    hipStream_t ls = lane ? h->stream2 : main;
    if (two_lanes)
      for (int d : op.xdeps) {
        le = hipStreamWaitEvent(ls, event_of((size_t)d), 0);
        if (le != hipSuccess) break;
      }
    if (le != hipSuccess) break;
    if (lp && std::find(lp->head.begin(), lp->head.end(), i) != lp->head.end()) le = launch_op(batch_part(op, 1, 2), P->arena, h->packed_dev, ls);
    else if (lp && lp->tail && i + 1 == nops) {
      le = launch_op(batch_part(op, 0, 2), P->arena, h->packed_dev, ls);
      if (le == hipSuccess) le = lp->mid_tail();
      if (le == hipSuccess) le = launch_op(batch_part(op, 1, 2), P->arena, h->packed_dev, ls);
    } else le = launch_op(op, P->arena, h->packed_dev, ls);
    if (le == hipSuccess && two_lanes && op.signal) le = hipEventRecord(event_of(i), ls);
  }
  if (two_lanes && le == hipSuccess) {
    le = hipEventRecord(event_of(nops + 1), h->stream2);
    if (le == hipSuccess) le = hipStreamWaitEvent(main, event_of(nops + 1), 0);
  } else if (two_lanes && !capturing) {
    // a launch or an event call failed behind the fork: the side stream may still hold lane-1 work that nothing on `main` is ordered
    // behind.  Drain it before the error goes back to the caller, who may reuse or free the buffers of this plan (round-5 ADVICE).
    // (inside a capture the streams carry no work: the capture itself is invalidated and ended by the caller)
    (void)hipStreamSynchronize(h->stream2);
  }
  return le == hipSuccess ? ev_err : le;
}

// Executes the plan on stream s (inputs already in the plan's img0 buffer, result left in its out buffer).
// n_ops < the plan's op count: only its first n_ops ops, in plan order on `s` alone (the pushed frame's extraction of a stream plan's first call).
int run_plan(film_t* h, Plan* P, hipStream_t s, size_t n_ops) {
  const int B = P->B, H = P->H, W = P->W;
  const bool prefix = n_ops < P->ops.size();
  if (h->opt_profile) {
    const size_t n = std::min(n_ops, P->ops.size());
    while (P->ev.size() < n + 1) { hipEvent_t e; HIPCHK(h, hipEventCreate(&e)); P->ev.push_back(e); }
    HIPCHK(h, hipEventRecord(P->ev[0], s));
    for (size_t i = 0; i < n; ++i) {
      HIPCHK(h, launch_op(P->ops[i], P->arena, h->packed_dev, s));
      HIPCHK(h, hipEventRecord(P->ev[i + 1], s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (!h->profile_append) { h->profile_ops.clear(); h->profile_classes.clear(); }   // (appending: one film_stream_push of several runs)
    auto& cls = h->profile_classes;
    std::ostringstream ops;
    for (size_t i = 0; i < n; ++i) {
      float ms = 0;
      HIPCHK(h, hipEventElapsedTime(&ms, P->ev[i], P->ev[i + 1]));
      film_t::ProfileClass& a = cls[kKindName[P->ops[i].kind]];
      a.launches++; a.ms += ms; a.flops += P->ops[i].flops; a.bytes += P->ops[i].bytes;
      ops << (i || !h->profile_ops.empty() ? "," : "") << "{\"tag\":\"" << P->ops[i].tag << "\",\"kind\":\"" << kKindName[P->ops[i].kind] << "\",\"ms\":" << ms
          << ",\"flops\":" << P->ops[i].flops << ",\"bytes\":" << P->ops[i].bytes << ",\"tile\":" << P->ops[i].tile << "}";
    }
    h->profile_ops += ops.str();
    std::ostringstream o;
    o << "{\"B\":" << B << ",\"H\":" << H << ",\"W\":" << W << ",\"classes\":{";
    bool first = true;
    for (auto& kv : cls) {
      o << (first ? "" : ",") << "\"" << kv.first << "\":{\"launches\":" << kv.second.launches << ",\"ms\":" << kv.second.ms
        << ",\"flops\":" << kv.second.flops << ",\"bytes\":" << kv.second.bytes << "}";
      first = false;
    }
    o << "},\"ops\":[" << h->profile_ops << "]}";
    h->profile_json = o.str();
  } else if (prefix) {
    for (size_t i = 0; i < n_ops; ++i) HIPCHK(h, launch_op(P->ops[i], P->arena, h->packed_dev, s));
  } else if (h->opt_graph == 1) {
    if (!P->graph_exec) {
      // capture on the handle's own stream, replay on whichever stream the caller wants
      HIPCHK(h, hipStreamSynchronize(s));
      HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
      const hipError_t le = issue_lanes(h, P, h->stream, true);
      hipError_t ce = hipStreamEndCapture(h->stream, &P->graph);
      if (le != hipSuccess) return fail(h, FILM_ERR_HIP, "kernel launch failed during capture: %s", hipGetErrorString(le));
      HIPCHK(h, ce);
      HIPCHK(h, hipGraphInstantiate(&P->graph_exec, P->graph, nullptr, nullptr, 0));
    }
    HIPCHK(h, hipGraphLaunch(P->graph_exec, s));
  } else if (h->opt_graph == 2 && h->opt_lanes != 0) {
    // the DEFAULT: the same two lanes and the same event edges, launched directly - lane 0 on the caller's stream, lane 1 on the
    // handle's side stream (issue_lanes; why not a hipGraph by default: film_internal.h, opt_graph)
    const hipError_t le = issue_lanes(h, P, s, false);
    if (le != hipSuccess) return fail(h, FILM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(le));
  } else {
    for (const OpDesc& op : P->ops) HIPCHK(h, launch_op(op, P->arena, h->packed_dev, s));
  }
  h->last_plan = P;
  return FILM_OK;
}

}  // namespace film_internal
