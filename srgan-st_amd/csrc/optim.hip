// Adam over ONE flat parameter buffer (replaces the multi-tensor launches of torch.optim.Adam(fused=True) that the
// step engines used before; reference train.py:62-75 / warmup.py:34-40 build torch.optim.Adam with eps 1e-4).
//
// The parameters of a network live in one flat fp32 buffer (srganst/ops.py: flatten_params), the gradients in a flat
// buffer of the same layout (flat_grads), so the update is a single streaming pass: 4 reads + 3 writes per element,
// HBM-bound.  Arithmetic follows torch's fused Adam kernel (non-amsgrad, maximize = False):
//   g' = g + wd * p;  m = lerp(m, g', 1 - b1);  v = b2 * v + (1 - b2) * g'^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// lr and the step counters are device memory, so the launch is hipGraph-capturable and LR schedulers keep working.
#include "common.h"
#include <cmath>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// steps[i] += 1 for the per-parameter step counters torch's state_dict exposes (all equal); separate tiny launch so that
// the update kernel's workgroups all see the same value.
__global__ void adam_tick_kernel(float* steps, int n) {
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
template <bool EMA>
__device__ __forceinline__ void adam_flat_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, float* __restrict__ ema, int64_t n4,
                                               const float* __restrict__ lr, const float* __restrict__ steps, double b1, double b2,
                                               double eps, double wd, double ema_decay, int ema_warmup) {
  __shared__ float s_c[2];
  __shared__ double s_d;
  if (threadIdx.x == 0) {
    const double t = (double)steps[0];
    const float bc1 = (float)(1.0 - pow(b1, t)), bc2 = (float)(1.0 - pow(b2, t));
    s_c[0] = (float)((double)lr[0] / (double)bc1);       // step size
    s_c[1] = sqrtf(bc2);
    if (EMA) s_d = ema_decay_at(t, ema_decay, ema_warmup);
  }
  __syncthreads();
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
