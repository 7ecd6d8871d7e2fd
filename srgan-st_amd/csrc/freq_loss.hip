// Focal frequency loss (loss.py: FocalFrequencyLoss; Jiang et al., ICCV 2021, the published defaults), forward and backward, for
// gfx950.  Per image and RGB plane, with d = sr - gt and Wh = W/2 + 1:
//
//   D[ky,kx] = (1/sqrt(HW)) sum_{y,x} d[y,x] exp(-2 pi i (ky y / H + kx x / W))        orthonormal 2-D DFT
//   e = |D|^2,  w = sqrt(e)^alpha / max over the plane of sqrt(e)^alpha   (NaN -> 0, clamped to [0,1], a constant for the gradient)
//   loss = mean over batch, planes and all H x W frequencies of w e
//   d loss / d sr = 2 / (B 3 H W) Re(F^H (w .* D))
//
// Only the half spectrum kx = 0 .. W/2 is computed (d is real: D[-ky,-kx] = conj D[ky,kx], so e and w repeat); in every sum over
// kx column 0 counts once, column W/2 once when W is even, every other column twice.
//
// Every transform is one kernel, freq_pass_kernel<MODE>: out[k][line] = sum_n in[line][n] tw[(k n) mod N], a direct DFT with runtime
// sizes (no radix restriction).  A workgroup takes 32 lines x 32 outputs k of one plane; the summation axis is staged through LDS in
// chunks of 128 (row pitch 129: lanes run along the lines, so the reads are conflict-free); a thread owns one line and four k, the k
// of a wave's half is uniform, so the twiddle reads are broadcasts, not gathers.  The table exp(-+2 pi i j / N) is built per
// workgroup in LDS from sincospi(2j/N) in fp64, rounded once; the index (k n) mod N runs and wraps in integers.  fp32 FMAs; the
// output tile is transposed through LDS so that every store is coalesced.
//
//   forward   1 ROW_FWD  sr, gt -> T[plane][kx][y]        (real to half spectrum along W)
//             2 COL_FWD  T -> Y[plane][ky][kx] = D        (complex along H, times 1/sqrt(HW); per-workgroup maximum of e)
//             3 weight   Y -> loss, and with saved != null saved[plane][ky][kx] = w .* D
//   backward  4 COL_ADJ  saved -> U[plane][y][kx]         (conjugate twiddles along H)
//             5 ROW_ADJ  U -> dsr                          (half spectrum to real along W, with the multiplicities)
//
// Kernel boundaries carry every cross-workgroup hand-off but the loss's: one fp64 partial per workgroup of kernel 3, summed in index
// order by the last-arriving workgroup, which re-arms the counter.  The plane maximum is order-independent.  No floating-point
// atomics: the same bits in every run and replay.
//
// NaN: a NaN in sr reaches every frequency of its plane; there w = NaN -> 0 and w e = NaN, so the loss is NaN and so is that
// plane's gradient - and nothing else.
#include "common.h"

#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int FNT = 256;               // threads per workgroup
constexpr int FL = 32;                 // lines per workgroup (lane & 31)
constexpr int FKB = 32;                // outputs k per workgroup: 8 thread groups x FNK
constexpr int FNK = 4;                 // outputs k per thread
constexpr int FNC = 128;               // summation chunk staged in LDS
constexpr int FP = FNC + 1;            // LDS row pitch of the staged chunk
constexpr int FMAXN = 512;             // largest H or W
constexpr int FWE = 1024;              // weight kernel: elements per workgroup

enum { ROW_FWD = 0, COL_FWD = 1, COL_ADJ = 2, ROW_ADJ = 3 };

struct PassArgs {
  int L, N, Nmod, K;                   // lines, summation length, twiddle modulus, outputs
  int64_t ld_in, ld_out, ps_in, ps_out;  // leading dimensions and plane strides, in elements of the respective array
};

// |D|^2 of one stored frequency: the column pass (for the maximum) and the weight kernel evaluate this one expression
__device__ __forceinline__ float spec_energy(float re, float im) { return fmaf(re, re, im * im); }

// sqrt(e)^alpha in fp64; alpha = 0 gives 1 for every e (pow(0, 0) = 1)
__device__ __forceinline__ double spec_pow(float e, double alpha) {
  if (alpha == 0.0) return 1.0;
  if (alpha == 1.0) return sqrt((double)e);
  if (alpha == 2.0) return (double)e;
  return pow(sqrt((double)e), alpha);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// in0 / in1: ROW_FWD sr / gt (fp32 planes), else in0 = the complex input (float2) and in1 unused.  out: complex (float2), ROW_ADJ: dsr.
// pmax (COL_FWD): [plane][gridDim.y * gridDim.x] maxima of e.  scale: COL_FWD 1/sqrt(HW); ROW_ADJ the gradient's host scale.
template <int MODE>
__global__ __launch_bounds__(FNT) void freq_pass_kernel(const float* __restrict__ in0, const float* __restrict__ in1,
                                                        float* __restrict__ out, float* __restrict__ pmax,
                                                        const float* __restrict__ scale_dev, double scale, int accumulate, PassArgs p) {
  constexpr bool REAL_IN = MODE == ROW_FWD, REAL_OUT = MODE == ROW_ADJ, INVERSE = MODE == COL_ADJ || MODE == ROW_ADJ;
  using TIn = typename std::conditional<REAL_IN, float, float2>::type;
  __shared__ TIn s_in[FL * FP];
  __shared__ float2 s_tw[FMAXN];
  __shared__ float2 s_out[FKB * (FL + 1)];
  __shared__ float s_red[FNT / 64];
  const int tid = threadIdx.x, l = tid & (FL - 1), kl = tid >> 5;
  const int l0 = blockIdx.x * FL, k0 = blockIdx.y * FKB;
  const int64_t z = blockIdx.z;
  const float2* cin = reinterpret_cast<const float2*>(in0) + z * p.ps_in;

  for (int j = tid; j < p.Nmod; j += FNT) {
    double s, c;
    sincospi(2.0 * (double)j / (double)p.Nmod, &s, &c);
    s_tw[j] = make_float2((float)c, (float)(INVERSE ? s : -s));
  }

  int kk[FNK], idx[FNK];
  float re[FNK], im[FNK];
#pragma unroll
  for (int j = 0; j < FNK; ++j) {
    const int k = k0 + kl + 8 * j;
    kk[j] = k < p.K ? k : 0;
    idx[j] = 0;
    re[j] = 0.f;
    im[j] = 0.f;
  }

  for (int n0 = 0; n0 < p.N; n0 += FNC) {
    const int nc = min(FNC, p.N - n0);
    __syncthreads();
    // ---- stage lines [l0, l0 + 32) x summation indices [n0, n0 + nc): zero beyond the last line
    for (int i = tid; i < FL * nc; i += FNT) {
      int ll, nn;
      if (MODE == COL_ADJ) {             // input [n][line]: consecutive threads along the lines
        ll = i & (FL - 1);
        nn = i >> 5;
      } else {                           // input [line][n]: consecutive threads along n
        ll = i / nc;
        nn = i - ll * nc;
      }
      const bool in = l0 + ll < p.L;
      if constexpr (REAL_IN) {
        const int64_t o = z * p.ps_in + (int64_t)(l0 + ll) * p.ld_in + (n0 + nn);
        s_in[ll * FP + nn] = in ? in0[o] - in1[o] : 0.f;
      } else {
        const int64_t o = MODE == COL_ADJ ? (int64_t)(n0 + nn) * p.ld_in + (l0 + ll) : (int64_t)(l0 + ll) * p.ld_in + (n0 + nn);
        float2 v = make_float2(0.f, 0.f);
        if (in) v = cin[o];
        if (MODE == ROW_ADJ) {           // the half spectrum's multiplicity: columns 0 and W/2 (W even) once, every other twice
          const int kx = n0 + nn;
          const float m = (kx == 0 || 2 * kx == p.Nmod) ? 1.f : 2.f;
          v.x *= m;
          v.y *= m;
        }
        s_in[ll * FP + nn] = v;
      }
    }
    __syncthreads();
    // ---- accumulate: one line, four k per thread; the twiddle index runs and wraps
    for (int n = 0; n < nc; ++n) {
      const TIn v = s_in[l * FP + n];
#pragma unroll
      for (int j = 0; j < FNK; ++j) {
        const float2 t = s_tw[idx[j]];
        if constexpr (REAL_IN) {
          re[j] = fmaf(v, t.x, re[j]);
          im[j] = fmaf(v, t.y, im[j]);
        } else {
          re[j] = fmaf(v.x, t.x, re[j]);
          re[j] = fmaf(-v.y, t.y, re[j]);
          if (!REAL_OUT) {
            im[j] = fmaf(v.x, t.y, im[j]);
            im[j] = fmaf(v.y, t.x, im[j]);
          }
        }
        idx[j] += kk[j];
        if (idx[j] >= p.Nmod) idx[j] -= p.Nmod;
      }
    }
  }

  // ---- transpose the 32 k x 32 line tile through LDS; every store below is coalesced
  const float fs = MODE == COL_FWD ? (float)scale : 1.f;
#pragma unroll
  for (int j = 0; j < FNK; ++j) s_out[(kl + 8 * j) * (FL + 1) + l] = make_float2(re[j] * fs, im[j] * fs);
  __syncthreads();

  if constexpr (REAL_OUT) {
    double sc = scale;
    if (scale_dev) sc = sc * (double)scale_dev[0];
    for (int i = tid; i < FL * FKB; i += FNT) {
      const int ll = i >> 5, kq = i & (FKB - 1);
      if (l0 + ll < p.L && k0 + kq < p.K) {
        const int64_t o = z * p.ps_out + (int64_t)(l0 + ll) * p.ld_out + (k0 + kq);
        const float vf = (float)((double)s_out[kq * (FL + 1) + ll].x * sc);
        out[o] = accumulate ? out[o] + vf : vf;
      }
    }
  } else {
    float2* cout = reinterpret_cast<float2*>(out) + z * p.ps_out;
    float emax = 0.f;
    for (int i = tid; i < FL * FKB; i += FNT) {
      const int kq = i >> 5, ll = i & (FL - 1);
      if (l0 + ll < p.L && k0 + kq < p.K) {
        const float2 v = s_out[kq * (FL + 1) + ll];
        cout[(int64_t)(k0 + kq) * p.ld_out + (l0 + ll)] = v;
        if (MODE == COL_FWD) emax = fmaxf(emax, spec_energy(v.x, v.y));
      }
    }
    if (MODE == COL_FWD) {
      emax = wave_max(emax);
      if ((tid & 63) == 0) s_red[tid >> 6] = emax;
      __syncthreads();
      if (tid == 0) {
#pragma unroll
        for (int k = 1; k < FNT / 64; ++k) emax = fmaxf(emax, s_red[k]);
        pmax[z * ((int64_t)gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x] = emax;
      }
    }
  }
}

// Y [plane][H][Wh] -> loss[0] = sum(mult w e) / count, and with saved != null saved = w .* Y.  grid (ceil(H Wh / 1024), planes).
__global__ __launch_bounds__(FNT) void freq_weight_kernel(const float2* __restrict__ Y, const float* __restrict__ pmax, int npm,
                                                          float2* __restrict__ saved, double* partials, unsigned* counter,
                                                          float* __restrict__ loss, int H, int W, double alpha, double count) {
  __shared__ double s_red[FNT / 64];
  __shared__ float s_max[FNT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x, Wh = W / 2 + 1, n = H * Wh;
  const int64_t z = blockIdx.y;

  // ---- the plane's maximum of e from the column pass's per-workgroup maxima (npm <= 144)
  float em = tid < npm ? pmax[z * npm + tid] : 0.f;
  em = wave_max(em);
  if ((tid & 63) == 0) s_max[tid >> 6] = em;
  __syncthreads();
  em = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  const double smax = spec_pow(em, alpha);

  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < FWE / FNT; ++j) {
    const int i = blockIdx.x * FWE + j * FNT + tid;
    if (i < n) {
      const int kx = i % Wh;
      const float2 v = Y[z * n + i];
      const float e = spec_energy(v.x, v.y);
      double w = spec_pow(e, alpha) / smax;
      if (!(w == w)) w = 0.0;                      // 0 / 0 (a plane with d = 0) and NaN input: weight 0; 0 * NaN stays NaN below
      w = fmin(fmax(w, 0.0), 1.0);
      const double m = (kx == 0 || 2 * kx == W) ? 1.0 : 2.0;
      ss += m * (w * (double)e);
      if (saved) saved[z * n + i] = make_float2((float)(w * (double)v.x), (float)(w * (double)v.y));
    }
  }

  // ---- one partial per workgroup; the last arriver sums them in index order and re-arms the counter
  const unsigned nblk = gridDim.x * gridDim.y;
  if (!last_block_arrive_d<FNT>(ss, partials, blockIdx.x + gridDim.x * blockIdx.y, counter, nblk, &s_flag, s_red)) return;
  const double t = last_block_total_d<FNT>(partials, counter, nblk, s_red);
  if (tid == 0) loss[0] = (float)(t / count);
}

// shape rules shared by the three entries
static int freq_check_shape(const char* who, int B, int H, int W) {
  SST_REQUIRE(B >= 1 && (int64_t)B * 3 <= 65535, "%s: bad batch %d", who, B);
  SST_REQUIRE(H >= 1 && H <= FMAXN && W >= 1 && W <= FMAXN, "%s: size %dx%d not built (1 <= H, W <= %d)", who, H, W, FMAXN);
  return SST_OK;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static int64_t freq_spec_floats(int B, int H, int W) { return (int64_t)B * 3 * H * (W / 2 + 1) * 2; }
static int freq_npm(int H, int W) { return cdiv(W / 2 + 1, FL) * cdiv(H, FKB); }          // column-pass workgroups per plane
static int freq_wblocks(int H, int W) { return cdiv(H * (W / 2 + 1), FWE); }              // weight-kernel workgroups per plane

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_freq_loss_workspace(int B, int H, int W, int64_t* saved_floats, int64_t* scratch_floats, int64_t* partial_floats) {
  SST_REQUIRE(saved_floats && scratch_floats && partial_floats, "sst_freq_loss_workspace: null pointer");
  if (int rc = freq_check_shape("sst_freq_loss_workspace", B, H, W)) return rc;
  const int64_t S = freq_spec_floats(B, H, W);
  *saved_floats = S;
  *scratch_floats = 2 * S + (int64_t)B * 3 * freq_npm(H, W);
  *partial_floats = 2 * (int64_t)B * 3 * freq_wblocks(H, W);            // one fp64 partial per workgroup of the weight kernel
  return SST_OK;
}

SST_API int sst_freq_loss_fwd(const float* sr, const float* gt, float* loss, float* saved, float* scratch, float* partials,
                              unsigned* counter, int B, int H, int W, double alpha, void* stream) {
  SST_REQUIRE(sr && gt && loss && scratch && partials && counter, "sst_freq_loss_fwd: null pointer");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0 && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(saved) & 7) == 0,
              "sst_freq_loss_fwd: saved, scratch and partials must be 8-byte aligned");
  if (int rc = freq_check_shape("sst_freq_loss_fwd", B, H, W)) return rc;
  SST_REQUIRE(std::isfinite(alpha) && alpha >= 0.0, "sst_freq_loss_fwd: alpha must be a finite number >= 0, got %g", alpha);
  const int planes = B * 3, Wh = W / 2 + 1;
  const int64_t S = freq_spec_floats(B, H, W), hw = (int64_t)H * W, hwh = (int64_t)H * Wh;
  float* T = scratch;
  float* Y = scratch + S;
  float* pmax = scratch + 2 * S;
  hipStream_t st = sst_stream(stream);
  {
    const PassArgs p{H, W, W, Wh, W, H, hw, hwh};
    freq_pass_kernel<ROW_FWD><<<dim3(cdiv(H, FL), cdiv(Wh, FKB), planes), FNT, 0, st>>>(sr, gt, T, nullptr, nullptr, 1.0, 0, p);
    SST_LAUNCH_CHECK("freq_pass_kernel<ROW_FWD>");
  }
  {
    const PassArgs p{Wh, H, H, H, H, Wh, hwh, hwh};
    freq_pass_kernel<COL_FWD><<<dim3(cdiv(Wh, FL), cdiv(H, FKB), planes), FNT, 0, st>>>(T, nullptr, Y, pmax, nullptr,
                                                                                         1.0 / std::sqrt((double)H * (double)W), 0, p);
    SST_LAUNCH_CHECK("freq_pass_kernel<COL_FWD>");
  }
  const double count = (double)B * 3.0 * (double)H * (double)W;
  freq_weight_kernel<<<dim3(freq_wblocks(H, W), planes), FNT, 0, st>>>(reinterpret_cast<const float2*>(Y), pmax, freq_npm(H, W),
                                                                      reinterpret_cast<float2*>(saved),
                                                                      reinterpret_cast<double*>(partials), counter, loss, H, W, alpha,
                                                                      count);
  SST_LAUNCH_CHECK("freq_weight_kernel");
  return SST_OK;
}

SST_API int sst_freq_loss_bwd(const float* saved, float* dsr, float* scratch, const float* scale_dev, float scale_host, int accumulate,
                              int B, int H, int W, void* stream) {
  SST_REQUIRE(saved && dsr && scratch, "sst_freq_loss_bwd: null pointer");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && (reinterpret_cast<uintptr_t>(saved) & 7) == 0,
              "sst_freq_loss_bwd: saved and scratch must be 8-byte aligned");
  if (int rc = freq_check_shape("sst_freq_loss_bwd", B, H, W)) return rc;
  const int planes = B * 3, Wh = W / 2 + 1;
  const int64_t hw = (int64_t)H * W, hwh = (int64_t)H * Wh;
  float* U = scratch;
  hipStream_t st = sst_stream(stream);
  {
    const PassArgs p{Wh, H, H, H, Wh, Wh, hwh, hwh};
    freq_pass_kernel<COL_ADJ><<<dim3(cdiv(Wh, FL), cdiv(H, FKB), planes), FNT, 0, st>>>(saved, nullptr, U, nullptr, nullptr, 1.0, 0, p);
    SST_LAUNCH_CHECK("freq_pass_kernel<COL_ADJ>");
  }
  {
    // d loss / d sr = 2 / (B 3 H W) * (1/sqrt(HW)) * sum over the half spectrum (the inverse transform's own normalisation)
    const double count = (double)B * 3.0 * (double)H * (double)W;
    const double scale = (double)scale_host * 2.0 / count / std::sqrt((double)H * (double)W);
    const PassArgs p{H, Wh, W, W, Wh, W, hwh, hw};
    freq_pass_kernel<ROW_ADJ><<<dim3(cdiv(H, FL), cdiv(W, FKB), planes), FNT, 0, st>>>(U, nullptr, dsr, nullptr, scale_dev, scale,
                                                                                        accumulate, p);
    SST_LAUNCH_CHECK("freq_pass_kernel<ROW_ADJ>");
  }
  return SST_OK;
}
