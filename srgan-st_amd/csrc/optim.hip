// Adam over ONE flat parameter buffer (replaces the multi-tensor launches of torch.optim.Adam(fused=True) that the
// step engines used before; reference train.py:62-75 / warmup.py:34-40 build torch.optim.Adam with eps 1e-4).
//
// The parameters of a network live in one flat fp32 buffer (srganst/ops.py: flatten_params), the gradients in a flat
// buffer of the same layout (flat_grads), so the update is a single streaming pass: 4 reads + 3 writes per element,
// HBM-bound.  Arithmetic follows torch's fused Adam kernel (non-amsgrad, maximize = False):
//   g' = g + wd * p;  m = lerp(m, g', 1 - b1);  v = b2 * v + (1 - b2) * g'^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// lr and the step counters are device memory, so the launch is hipGraph-capturable and LR schedulers keep working.
//
// Global gradient-norm clipping and the non-finite guard (sst_grad_sumsq + sst_adam_flat_clip) ride on the same buffers: one
// fixed-order fp64 reduction of the gradient's parameter elements (pad words are never read), then the single-workgroup tick
// kernel turns the partials into a device record (norm, coefficient, skip decision, cumulative counters) that every workgroup
// of the update reads.  No atomics and no cross-workgroup ordering anywhere: bit-reproducible, eager or replayed.
#include "common.h"
#include <cmath>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// steps[i] += 1 for the per-parameter step counters torch's state_dict exposes (all equal); separate tiny launch so that
// the update kernel's workgroups all see the same value.
__global__ void adam_tick_kernel(float* steps, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) steps[i] += 1.f;
}

// The device record sst_adam_flat_clip keeps (doubles; the counters are whole numbers, exact far beyond any run's length).
enum { REC_NORM = 0, REC_COEF = 1, REC_SKIPPED_NOW = 2, REC_N_SKIPPED = 3, REC_N_CLIPPED = 4, REC_N_STEPS_SEEN = 5, REC_WORDS = 6 };

// Sum of squares of ONE job (start, count) of the flat gradient buffer, in fp64: each fp32 value is widened before it is squared
// (24-bit significands: the square is exact in double), per-thread sums in a fixed order, then wave shuffle -> LDS -> one plain
// store per workgroup.  Only [start, start + count) is read: a job never covers a pad word (optim.norm_jobs).  float4 loads from
// the first 16-byte boundary on, scalar head and tail.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const int64_t* __restrict__ jobs,
                                                         double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t start = jobs[2 * (int64_t)blockIdx.x], count = jobs[2 * (int64_t)blockIdx.x + 1];
  const float* __restrict__ s = g + start;
  int64_t head = (4 - (start & 3)) & 3;
  if (head > count) head = count;
  const int64_t nvec = (count - head) >> 2, tail = head + 4 * nvec;
  double acc = 0.0;
  if ((int64_t)threadIdx.x < head) {
    const double x = (double)s[threadIdx.x];
    acc += x * x;
  }
  const f32x4* __restrict__ s4 = reinterpret_cast<const f32x4*>(s + head);
  for (int64_t i = threadIdx.x; i < nvec; i += 256) {
    const f32x4 q = s4[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = (double)q[j];
      acc += x * x;
    }
  }
  for (int64_t i = tail + threadIdx.x; i < count; i += 256) {
    const double x = (double)s[i];
    acc += x * x;
  }
  const double total = block_sum_d<256>(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// adam_tick_kernel with the clip rule: sums the partials in a fixed order, writes the record and ticks the step counters unless
// the step is skipped.  coef = min(1, max_norm / (norm + 1e-6)) in double, rounded once to fp32 (torch.nn.utils.clip_grad_norm_);
// the min lets NaN through like torch.clamp does (guard off and a NaN gradient: the update poisons the parameters, as torch's
// does with error_if_nonfinite=False).  max_norm == 0: no clipping, coef = 1.
__global__ __launch_bounds__(256) void adam_clip_tick_kernel(float* steps, int n, const double* __restrict__ partials, int npartials,
                                                             double max_norm, int skip_nonfinite, double* __restrict__ rec) {
  __shared__ double red[4];
  double t = 0.0;
  for (int i = threadIdx.x; i < npartials; i += 256) t += partials[i];
  const double sum = block_sum_d<256>(t, red);
  const bool skip = skip_nonfinite && !isfinite(sum);
  if (threadIdx.x == 0) {
    const double norm = sqrt(sum);
    float coef = 1.f;
    if (max_norm > 0.0) {
      const double c = max_norm / (norm + 1e-6);
      coef = (float)(c >= 1.0 ? 1.0 : c);              // c NaN: stays NaN
    }
    rec[REC_NORM] = norm;
    rec[REC_COEF] = (double)coef;
    rec[REC_SKIPPED_NOW] = skip ? 1.0 : 0.0;
    rec[REC_N_SKIPPED] += skip ? 1.0 : 0.0;
    rec[REC_N_CLIPPED] += (!skip && coef < 1.f) ? 1.0 : 0.0;
    rec[REC_N_STEPS_SEEN] += 1.0;
  }
  if (skip) return;
  for (int i = threadIdx.x; i < n; i += blockDim.x) steps[i] += 1.f;
}

// The decay of the parameter average at Adam step t (1 at the first update): with warm-up the average follows the parameters
// closely while t is small, d = min(decay, (1 + t) / (10 + t)); without, d = decay.  Double, like every constant here.
__device__ __forceinline__ double ema_decay_at(double t, double decay, int warmup) {
  if (!warmup) return decay;
  const double w = (1.0 + t) / (10.0 + t);
  return w < decay ? w : decay;
}

// One element of the average: d * ema + (1 - d) * p in double, rounded to fp32 once.  The fma is spelled out so that both
// kernels that apply the rule round the same way whatever the compiler contracts around them.
__device__ __forceinline__ float ema_step(double d, double wp, float ema, float p) {
  return (float)fma(d, (double)ema, wp * (double)p);
}

// Constants are doubles and the moment updates are evaluated in double before rounding to fp32, as in torch's kernel
// (its betas / eps / lr are double arguments): with float constants (1 - 0.999f) is already off by 5e-5 relative.
// EMA: the same pass also moves an exponential average of the parameters towards the NEW p (one more read + write per
// element, 36 B instead of 28 B); evaluated in double and rounded once, like the moments.  p / m / v do not depend on it.
// CLIP: every workgroup reads the coefficient and the skip decision from the record the tick kernel wrote.  On skip nothing is
// touched; otherwise an element's gradient is g * coef - ONE fp32 multiply, rounded before weight decay or anything else sees it
// (__fmul_rn: never contracted), exact when coef == 1.
template <bool EMA, bool CLIP = false>
__device__ __forceinline__ void adam_flat_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, float* __restrict__ ema, int64_t n4,
                                               const float* __restrict__ lr, const float* __restrict__ steps, double b1, double b2,
                                               double eps, double wd, double ema_decay, int ema_warmup,
                                               const double* __restrict__ rec = nullptr) {
  __shared__ float s_c[2];
  __shared__ double s_d;
  __shared__ float s_coef;
  __shared__ int s_skip;
  if (threadIdx.x == 0) {
    if (CLIP) {
      s_coef = (float)rec[REC_COEF];
      s_skip = rec[REC_SKIPPED_NOW] != 0.0;
    }
    const double t = (double)steps[0];
    const float bc1 = (float)(1.0 - pow(b1, t)), bc2 = (float)(1.0 - pow(b2, t));
    s_c[0] = (float)((double)lr[0] / (double)bc1);       // step size
    s_c[1] = sqrtf(bc2);
    if (EMA) s_d = ema_decay_at(t, ema_decay, ema_warmup);
  }
  __syncthreads();
  if (CLIP && s_skip) return;
  const float coef = CLIP ? s_coef : 1.f;
  const float step_size = s_c[0], bc2_sqrt = s_c[1];
  const double w1 = 1.0 - b1, w2 = 1.0 - b2;
  const double d = EMA ? s_d : 0.0, wp = 1.0 - d;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ev;
    if (EMA) ev = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gg = gv[j];
      if (CLIP) gg = __fmul_rn(gg, coef);
      if (wd != 0.0) gg = (float)((double)gg + (double)pv[j] * wd);
      mv[j] = (float)(b1 * (double)mv[j] + w1 * (double)gg);
      vv[j] = (float)(b2 * (double)vv[j] + w2 * (double)gg * (double)gg);
      const float denom = (float)((double)(sqrtf(vv[j]) / bc2_sqrt) + eps);
      pv[j] -= step_size * mv[j] / denom;
      if (EMA) ev[j] = ema_step(d, wp, ev[j], pv[j]);
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if (EMA) reinterpret_cast<f32x4*>(ema)[i] = ev;
  }
}

__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n4, const float* __restrict__ lr,
                                                        const float* __restrict__ steps, double b1, double b2, double eps,
                                                        double wd) {
  adam_flat_body<false>(p, g, m, v, nullptr, n4, lr, steps, b1, b2, eps, wd, 0.0, 0);
}

__global__ __launch_bounds__(256) void adam_flat_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, float* __restrict__ ema, int64_t n4,
                                                            const float* __restrict__ lr, const float* __restrict__ steps, double b1,
                                                            double b2, double eps, double wd, double ema_decay, int ema_warmup) {
  adam_flat_body<true>(p, g, m, v, ema, n4, lr, steps, b1, b2, eps, wd, ema_decay, ema_warmup);
}

__global__ __launch_bounds__(256) void adam_flat_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, int64_t n4, const float* __restrict__ lr,
                                                             const float* __restrict__ steps, double b1, double b2, double eps,
                                                             double wd, const double* __restrict__ rec) {
  adam_flat_body<false, true>(p, g, m, v, nullptr, n4, lr, steps, b1, b2, eps, wd, 0.0, 0, rec);
}

__global__ __launch_bounds__(256) void adam_flat_ema_clip_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                 float* __restrict__ m, float* __restrict__ v, float* __restrict__ ema,
                                                                 int64_t n4, const float* __restrict__ lr,
                                                                 const float* __restrict__ steps, double b1, double b2, double eps,
                                                                 double wd, double ema_decay, int ema_warmup,
                                                                 const double* __restrict__ rec) {
  adam_flat_body<true, true>(p, g, m, v, ema, n4, lr, steps, b1, b2, eps, wd, ema_decay, ema_warmup, rec);
}

// The average's update alone (same rule, same rounding as in adam_flat_ema_kernel), for steps whose Adam update is not ours.
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n4,
                                                       const float* __restrict__ steps, double ema_decay, int ema_warmup) {
  __shared__ double s_d;
  if (threadIdx.x == 0) s_d = ema_decay_at((double)steps[0], ema_decay, ema_warmup);
  __syncthreads();
  const double d = s_d, wp = 1.0 - d;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
    f32x4 ev = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[j] = ema_step(d, wp, ev[j], pv[j]);
    reinterpret_cast<f32x4*>(ema)[i] = ev;
  }
}

inline int flat_blocks(int64_t n4) { return (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096); }

}  // namespace

// p, g, m, v: flat fp32 buffers of n floats (n % 4 == 0, 16-byte aligned).  Pad words between the parameter slots are updated
// like any other element and are don't-care: flatten_params zeroes them in p, flat_grads leaves them uninitialised in g, and
// whatever they hold (NaN included) stays confined to the pad words of p / m / v - no parameter element ever reads one.  steps: nsteps device floats (all incremented by one,
// steps[0] is the t of this update).  lr: device scalar.
SST_API int sst_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, const float* lr, float* steps, int nsteps,
                          double beta1, double beta2, double eps, double weight_decay, void* stream) {
  SST_REQUIRE(p && g && m && v && lr && steps && n > 0 && (n & 3) == 0 && nsteps > 0, "sst_adam_flat: bad argument");
  hipStream_t st = sst_stream(stream);
  adam_tick_kernel<<<1, 256, 0, st>>>(steps, nsteps);
  SST_LAUNCH_CHECK("adam_tick_kernel");
  const int64_t n4 = n >> 2;
  adam_flat_kernel<<<flat_blocks(n4), 256, 0, st>>>(p, g, m, v, n4, lr, steps, beta1, beta2, eps, weight_decay);
  SST_LAUNCH_CHECK("adam_flat_kernel");
  return SST_OK;
}

// sst_adam_flat plus, in the same pass, ema = d * ema + (1 - d) * p_new with d = ema_decay, or min(ema_decay, (1 + t) / (10 + t))
// with ema_warmup (t = steps[0] after the tick).  ema: n floats in p's layout; p / m / v come out as from sst_adam_flat.
SST_API int sst_adam_flat_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* lr, float* steps,
                              int nsteps, double beta1, double beta2, double eps, double weight_decay, double ema_decay,
                              int ema_warmup, void* stream) {
  SST_REQUIRE(p && g && m && v && ema && lr && steps && n > 0 && (n & 3) == 0 && nsteps > 0, "sst_adam_flat_ema: bad argument");
  SST_REQUIRE(ema_decay >= 0.0 && ema_decay <= 1.0, "sst_adam_flat_ema: ema_decay outside [0, 1]");
  hipStream_t st = sst_stream(stream);
  adam_tick_kernel<<<1, 256, 0, st>>>(steps, nsteps);
  SST_LAUNCH_CHECK("adam_tick_kernel");
  const int64_t n4 = n >> 2;
  adam_flat_ema_kernel<<<flat_blocks(n4), 256, 0, st>>>(p, g, m, v, ema, n4, lr, steps, beta1, beta2, eps, weight_decay, ema_decay,
                                                        ema_warmup);
  SST_LAUNCH_CHECK("adam_flat_ema_kernel");
  return SST_OK;
}

// The average's update alone: no tick, no Adam; t = steps[0] as it stands (after the update that produced p).
SST_API int sst_ema_flat(float* ema, const float* p, int64_t n, const float* steps, double ema_decay, int ema_warmup, void* stream) {
  SST_REQUIRE(ema && p && steps && n > 0 && (n & 3) == 0, "sst_ema_flat: bad argument");
  SST_REQUIRE(ema_decay >= 0.0 && ema_decay <= 1.0, "sst_ema_flat: ema_decay outside [0, 1]");
  const int64_t n4 = n >> 2;
  ema_flat_kernel<<<flat_blocks(n4), 256, 0, sst_stream(stream)>>>(ema, p, n4, steps, ema_decay, ema_warmup);
  SST_LAUNCH_CHECK("ema_flat_kernel");
  return SST_OK;
}

// Sum of squares of the parameter elements of a flat gradient buffer: workgroup j reduces job j = (start, count) of the table and
// stores partials[j] (fp64).  jobs: njobs int64 pairs on the device; jobs_host: the same table in host memory, checked here (no
// job may be empty, start before 0 or reach past n) before anything is launched.  Bit-reproducible.
SST_API int sst_grad_sumsq(const float* g, int64_t n, const int64_t* jobs, const int64_t* jobs_host, int njobs, double* partials,
                           void* stream) {
  SST_REQUIRE(g && jobs && jobs_host && partials, "sst_grad_sumsq: null pointer");
  SST_REQUIRE(n > 0 && (n & 3) == 0 && njobs > 0, "sst_grad_sumsq: bad argument (n = %lld must be a positive multiple of 4, njobs = %d)",
              (long long)n, njobs);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(g) & 15) == 0, "sst_grad_sumsq: g must be 16-byte aligned");
  for (int j = 0; j < njobs; ++j) {
    const int64_t start = jobs_host[2 * j], count = jobs_host[2 * j + 1];
    SST_REQUIRE(start >= 0 && count > 0 && start <= n && count <= n - start,
                "sst_grad_sumsq: job %d (start %lld, count %lld) reaches outside the buffer of %lld floats", j, (long long)start,
                (long long)count, (long long)n);
  }
  grad_sumsq_kernel<<<njobs, 256, 0, sst_stream(stream)>>>(g, jobs, partials);
  SST_LAUNCH_CHECK("grad_sumsq_kernel");
  return SST_OK;
}

// sst_adam_flat (ema == NULL) / sst_adam_flat_ema with global gradient-norm clipping and the non-finite guard, two launches:
//   1. the tick kernel sums partials[0 .. npartials) (sst_grad_sumsq's output for this g) in a fixed order and writes rec:
//      norm = sqrt(sum), coef = (float)min(1, max_norm / (norm + 1e-6)) (max_norm == 0: 1), skipped_now = skip_nonfinite && the sum
//      is not finite, and the cumulative n_skipped, n_clipped, n_steps_seen; the step counters tick only when not skipping;
//   2. the update: untouched p / m / v / ema on skip, else today's body on g * coef (one fp32 multiply).  coef == 1 gives the bits
//      of sst_adam_flat / sst_adam_flat_ema.
// rec: 6 device doubles, zeroed once by the caller (the counters accumulate).
SST_API int sst_adam_flat_clip(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* lr, float* steps,
                               int nsteps, double beta1, double beta2, double eps, double weight_decay, double ema_decay,
                               int ema_warmup, const double* partials, int npartials, double max_norm, int skip_nonfinite,
                               double* rec, void* stream) {
  SST_REQUIRE(p && g && m && v && lr && steps && partials && rec, "sst_adam_flat_clip: null pointer");
  SST_REQUIRE(n > 0 && (n & 3) == 0 && nsteps > 0 && npartials > 0,
              "sst_adam_flat_clip: bad argument (n = %lld must be a positive multiple of 4)", (long long)n);
  SST_REQUIRE(max_norm >= 0.0, "sst_adam_flat_clip: max_norm must be >= 0 (0 = no clipping)");      // false for NaN too
  SST_REQUIRE(!ema || (ema_decay >= 0.0 && ema_decay <= 1.0), "sst_adam_flat_clip: ema_decay outside [0, 1]");
  hipStream_t st = sst_stream(stream);
  adam_clip_tick_kernel<<<1, 256, 0, st>>>(steps, nsteps, partials, npartials, max_norm, skip_nonfinite ? 1 : 0, rec);
  SST_LAUNCH_CHECK("adam_clip_tick_kernel");
  const int64_t n4 = n >> 2;
  if (ema)
    adam_flat_ema_clip_kernel<<<flat_blocks(n4), 256, 0, st>>>(p, g, m, v, ema, n4, lr, steps, beta1, beta2, eps, weight_decay,
                                                               ema_decay, ema_warmup, rec);
  else
    adam_flat_clip_kernel<<<flat_blocks(n4), 256, 0, st>>>(p, g, m, v, n4, lr, steps, beta1, beta2, eps, weight_decay, rec);
  SST_LAUNCH_CHECK("adam_flat_clip_kernel");
  return SST_OK;
}
