// film_metrics.cpp -- film_image_metrics (include/film_hip.h): argument checks, scratch, copies and the host-side last step of the
// per-image evaluation metrics whose kernels are in metrics_kernels.hip (eval/metrics.py; reference losses/losses.py:72-113).
#include "film_internal.h"

using namespace film_internal;

namespace {

// metrics._gauss_window(11, 1.5): g = exp(-(x^2) / (2 sigma^2) - max) / sum, the sum in numpy's pairwise order for 11 values
// (eight partial sums combined as a tree, then the last three)
void gauss_window(double g[FILM_SSIM_TAPS], double sigma) {
  double mx = -INFINITY;
  for (int i = 0; i < FILM_SSIM_TAPS; ++i) {
    const double x = i - (FILM_SSIM_TAPS - 1) / 2.0;
    g[i] = -(x * x) / (2.0 * sigma * sigma);
    mx = std::max(mx, g[i]);
  }
  for (int i = 0; i < FILM_SSIM_TAPS; ++i) g[i] = std::exp(g[i] - mx);
  double sum = ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]));
  for (int i = 8; i < FILM_SSIM_TAPS; ++i) sum += g[i];
  for (int i = 0; i < FILM_SSIM_TAPS; ++i) g[i] /= sum;
}

}  // namespace

extern "C" int film_image_metrics(film_t* h, const float* pred, const float* ref, int B, int H, int W, int C, int flags,
                                  double max_val, double* out, int mem_kind, void* stream) {
  constexpr int kAll = FILM_METRIC_L1 | FILM_METRIC_L2 | FILM_METRIC_PSNR | FILM_METRIC_SSIM | FILM_METRIC_CLIP;
  if (!h || !pred || !ref || !out) return fail(h, FILM_ERR_INVALID, "NULL argument");
  if (B <= 0 || H <= 0 || W <= 0) return fail(h, FILM_ERR_INVALID, "B, H, W must be positive (got %d, %d, %d)", B, H, W);
  if (C != 1 && C != 3) return fail(h, FILM_ERR_INVALID, "C must be 1 or 3 (got %d)", C);
  if (!(max_val > 0)) return fail(h, FILM_ERR_INVALID, "max_val must be positive (got %g)", max_val);
  if (flags & ~kAll) return fail(h, FILM_ERR_INVALID, "unknown metric flags 0x%x", flags & ~kAll);
  if ((flags & FILM_METRIC_SSIM) && (H < FILM_SSIM_TAPS || W < FILM_SSIM_TAPS))
    return fail(h, FILM_ERR_INVALID, "ssim needs images of at least %d x %d (got %d x %d)", FILM_SSIM_TAPS, FILM_SSIM_TAPS, H, W);
  if (mem_kind != FILM_MEM_HOST && mem_kind != FILM_MEM_DEVICE) return fail(h, FILM_ERR_INVALID, "bad mem_kind");
  if (h->plan_only) return fail(h, FILM_ERR_NO_DEVICE, "plan-only handle: film_image_metrics needs a HIP device (no CPU fallback)");
  HIPCHK(h, hipSetDevice(h->device));
  // stream == NULL: as film_forward - the handle's stream for host buffers, the NULL stream for device buffers
  const hipStream_t s = stream ? (hipStream_t)stream : (mem_kind == FILM_MEM_DEVICE ? (hipStream_t) nullptr : h->stream);

  MetricsParams p{};
  p.B = B; p.H = H; p.W = W; p.C = C; p.flags = flags;
  gauss_window(p.g, 1.5);
  p.c1 = std::pow(0.01 * max_val, 2.0);
  p.c2 = std::pow(0.03 * max_val, 2.0);
  film_metrics_layout(p);
  const size_t n = (size_t)B * H * W * C;                   // floats per input
  const size_t part_bytes = (size_t)B * p.part_per_image * sizeof(double), out_bytes = (size_t)B * 4 * sizeof(double);
  const size_t need = part_bytes + out_bytes + (mem_kind == FILM_MEM_HOST ? 2 * n * sizeof(float) : 0);
  if (need > h->metrics_bytes) {
    if (h->metrics_buf) HIPCHK(h, hipFree(h->metrics_buf));   // nothing uses it: every call synchronises before it returns
    h->metrics_buf = nullptr;
    h->metrics_bytes = 0;
    if (hipMalloc(&h->metrics_buf, need) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, FILM_ERR_NOMEM, "film_image_metrics: cannot allocate %.1f MB of scratch", need * 1e-6);
    }
    h->metrics_bytes = need;
  }
  char* base = static_cast<char*>(h->metrics_buf);
  p.part = reinterpret_cast<double*>(base);
  p.out = reinterpret_cast<double*>(base + part_bytes);
  if (mem_kind == FILM_MEM_HOST) {
    float* st = reinterpret_cast<float*>(base + part_bytes + out_bytes);
    HIPCHK(h, hipMemcpyAsync(st, pred, n * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(st + n, ref, n * sizeof(float), hipMemcpyHostToDevice, s));
    p.pred = st;
    p.ref = st + n;
  } else {
    p.pred = pred;
    p.ref = ref;
  }
  HIPCHK(h, film_launch_image_metrics(p, s));
  std::vector<double> sums((size_t)B * 4);
  HIPCHK(h, hipMemcpyAsync(sums.data(), p.out, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));

  const double nan = std::nan(""), per_image = (double)H * W * C;
  for (int k = 0; k < B; ++k) {
    const double* v = &sums[(size_t)k * 4];
    double* o = out + (size_t)k * 4;
    o[0] = (flags & FILM_METRIC_L1) ? v[0] : nan;
    o[1] = (flags & FILM_METRIC_L2) ? v[1] : nan;
    // metrics.psnr: 20 log10(max_val) - 10 log10(mse), +inf for mse = 0
    o[2] = (flags & FILM_METRIC_PSNR) ? 20.0 * std::log10(max_val) - 10.0 * std::log10(v[2] / per_image) : nan;
    o[3] = (flags & FILM_METRIC_SSIM) ? v[3] : nan;
  }
  return FILM_OK;
}
