// The artifact-map (locally discriminative, "LDL") loss of Liang et al., "Details or Artifacts" (CVPR 2022), as a criterion
// (loss.py: ArtifactLoss), forward and backward, for gfx950.  sr, gt and the optional ref (the averaged generator's output for the
// same LR batch) are fp32 [B,3,H,W]; k = ksize is odd, 3..11, p = k / 2:
//
//   r   = |gt - sr| summed over R, G, B in that order, r_e the same of ref                                       [B,1,H,W]
//   s_b = (the unbiased variance of r over the H*W pixels of image b)^(1/5)                                      the global weight
//   v   = the unbiased variance (divisor k*k - 1) of the k x k window of r around the pixel, r reflect-padded by p (index -i reads
//         i, H-1+i reads H-1-i, as F.pad(mode="reflect"))                                                       the local weight
//   w   = s_b v, and 0 where r < r_e strictly (only with ref)
//   loss = mean over B*3*H*W of w |sr - gt|;   w is a constant of the gradient:  d loss / d sr = w sign(sr - gt) / (3 B H W)
//
// Arithmetic: the loads are fp32, everything after them fp64 - r and r_e (two adds of three exact-to-rounding differences, no
// multiply, so nothing for the compiler to fuse: the same bits as the fp64 restatement, and with them the same mask), both
// variances, the comparison, the loss sum.  Both variances are sums of d and d*d of SHIFTED data, d = r - c with c a value of the
// data itself (the image's first pixel for s_b, the window's centre for v): a constant residual gives d = 0 everywhere and a
// variance of exactly 0, and the subtraction S2 - S1^2 / n cancels at most about log2(n) bits.  A variance that rounds below zero
// is set to zero by a comparison that keeps a NaN.  sr == gt: r = 0, s_b = 0, w = 0 - a loss of exactly 0, a gradient of exactly 0.
//
// Forward, two launches over the same grid, one workgroup per 32 x 32 tile and image:
//   artifact_stats_kernel   (S1, S2) of the tile's pixels as two fp64 partials; the last-arriving workgroup (common.h) totals each
//                           image's partials in a fixed order (a wave per image, lane l adds partials l, l + 64, ...; then the wave
//                           sum), writes the B global weights behind the partials and re-arms its counter.
//   artifact_loss_fwd_kernel<k>  r of the tile with a p-wide ring in LDS (fp64, (32 + 2p)^2 values: 14 KB at k = 11), the
//                           reflection resolved on load - also where the ring leaves the image inside a partial tile; the window
//                           sums, w, the mask (ref is read on the tile only), w as one float per pixel where a gradient is wanted,
//                           and w r reduced by the fp64 last-arriver pieces.  No floating-point atomics: the same bits in every
//                           run and graph replay.
// Backward, one launch: dsr (+)= scale w sign(sr - gt), one thread per element; sign(0) = 0, sign(NaN) = NaN.
//
// NaN: a NaN in sr makes r NaN at its pixel, so its image's s_b, every w of that image that is not masked and the loss are NaN; the
// other images keep their bits.
#include "common.h"

#include <cmath>

namespace {

constexpr int AT = 32;                 // tile edge
constexpr int ANT = 256;
constexpr int AMAXK = 11;

// r at one pixel: the channel sum in the order R, G, B
__device__ __forceinline__ double residual(const float* __restrict__ a, const float* __restrict__ b, int64_t hw, int64_t o) {
  const double d0 = fabs((double)a[o] - (double)b[o]);
  const double d1 = fabs((double)a[o + hw] - (double)b[o + hw]);
  const double d2 = fabs((double)a[o + 2 * hw] - (double)b[o + 2 * hw]);
  return (d0 + d1) + d2;
}

// index i of an axis of n reflect-padded by at most n - 1: -i reads i, n - 1 + i reads n - 1 - i
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// stats (fp64): [0, nblk) S1 per tile, [nblk, 2 nblk) S2 per tile, [2 nblk, 2 nblk + B) the global weights
__global__ __launch_bounds__(ANT) void artifact_stats_kernel(const float* __restrict__ sr, const float* __restrict__ gt, double* stats,
                                                             unsigned* counter, int H, int W) {
  __shared__ double s_red[ANT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * AT, y0 = blockIdx.y * AT;
  const int64_t hw = (int64_t)H * W;
  const float* xs = sr + (int64_t)b * 3 * hw;
  const float* xg = gt + (int64_t)b * 3 * hw;
  const double c = residual(xg, xs, hw, 0);                    // the shift: r of the image's first pixel
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < AT * AT; i += ANT) {
    const int y = y0 + i / AT, x = x0 + i % AT;
    if (y < H && x < W) {
      const double d = residual(xg, xs, hw, (int64_t)y * W + x) - c;
      s1 += d;
      s2 += d * d;
    }
  }
  const unsigned per_img = gridDim.x * gridDim.y, nblk = per_img * gridDim.z;
  const unsigned blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  s2 = block_sum_d<ANT>(s2, s_red);
  if (tid == 0) stats[nblk + blk] = s2;                        // published by the release in front of thread 0's ticket below
  __syncthreads();                                             // s_red is free again
  if (!last_block_arrive_d<ANT>(s1, stats, blk, counter, nblk, &s_flag, s_red)) return;
  const double n = (double)H * (double)W;
  const int lane = tid & 63;
  for (unsigned img = tid >> 6; img < gridDim.z; img += ANT / 64) {
    double t1 = 0.0, t2 = 0.0;
    for (unsigned k = lane; k < per_img; k += 64) {
      t1 += load_agent_d(stats + (int64_t)img * per_img + k);
      t2 += load_agent_d(stats + (int64_t)nblk + (int64_t)img * per_img + k);
    }
    t1 = wave_sum_d(t1);
    t2 = wave_sum_d(t2);
    if (lane == 0) {
      double var = (t2 - t1 * (t1 / n)) / (n - 1.0);
      var = var < 0.0 ? 0.0 : var;                             // rounding only; a NaN stays
      stats[2 * (int64_t)nblk + img] = pow(var, 0.2);
    }
  }
  if (tid == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int K>
__global__ __launch_bounds__(ANT) void artifact_loss_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                                const float* __restrict__ ref, const double* __restrict__ weights,
                                                                float* __restrict__ wmap, double* partials, unsigned* counter,
                                                                float* __restrict__ loss, int H, int W, double count) {
  constexpr int P = K / 2, S = AT + 2 * P;                     // ring width, side (and row pitch) of the staged tile
  __shared__ double s_r[S * S];
  __shared__ double s_red[ANT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * AT, y0 = blockIdx.y * AT;
  const int64_t hw = (int64_t)H * W;
  const float* xs = sr + (int64_t)b * 3 * hw;
  const float* xg = gt + (int64_t)b * 3 * hw;
  // ---- r on the tile plus its ring; positions no pixel of the image reads (more than P beyond the last row or column) hold zero
  for (int i = tid; i < S * S; i += ANT) {
    const int ry = i / S, rx = i - ry * S;
    const int gy = y0 - P + ry, gx = x0 - P + rx;
    double v = 0.0;
    if (gy < H + P && gx < W + P) v = residual(xg, xs, hw, (int64_t)reflect(gy, H) * W + reflect(gx, W));
    s_r[i] = v;
  }
  __syncthreads();
  const double sb = weights[b];
  constexpr double inv_n = 1.0 / (double)(K * K), inv_nm1 = 1.0 / (double)(K * K - 1);
  double ss = 0.0;
  for (int i = tid; i < AT * AT; i += ANT) {
    const int j = i / AT, c = i % AT;
    const int y = y0 + j, x = x0 + c;
    if (y >= H || x >= W) continue;
    const double* win = s_r + j * S + c;                       // the window's top-left corner
    const double r = win[P * S + P];
    double s1 = 0.0, s2 = 0.0;
    for (int dy = 0; dy < K; ++dy) {
#pragma unroll
      for (int dx = 0; dx < K; ++dx) {
        const double d = win[dy * S + dx] - r;
        s1 += d;
        s2 += d * d;
      }
    }
    double v = (s2 - s1 * (s1 * inv_n)) * inv_nm1;
    v = v < 0.0 ? 0.0 : v;                                     // rounding only; a NaN stays
    double w = sb * v;
    const int64_t o = (int64_t)y * W + x;
    if (ref) {
      const double re = residual(xg, ref + (int64_t)b * 3 * hw, hw, o);
      if (r < re) w = 0.0;
    }
    if (wmap) wmap[(int64_t)b * hw + o] = (float)w;
    ss += w * r;
  }
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const unsigned blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (!last_block_arrive_d<ANT>(ss, partials, blk, counter, nblk, &s_flag, s_red)) return;
  const double t = last_block_total_d<ANT>(partials, counter, nblk, s_red);
  if (tid == 0) loss[0] = (float)(t / count);
}

// dsr (+)= scale * (scale_dev ? *scale_dev : 1) * w * sign(sr - gt);  scale = scale_host / (3 B H W)
__global__ __launch_bounds__(ANT) void artifact_loss_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                                const float* __restrict__ wmap, float* __restrict__ dsr,
                                                                const float* __restrict__ scale_dev, double scale, int accumulate,
                                                                int64_t hw, int64_t total) {
  const int64_t q = (int64_t)blockIdx.x * ANT + threadIdx.x;
  if (q >= total) return;
  double sc = scale;
  if (scale_dev) sc = sc * (double)scale_dev[0];
  const int64_t b = q / (3 * hw), pix = q % hw;
  const double d = (double)sr[q] - (double)gt[q];
  const double sgn = d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d;       // a tie gives 0, a NaN stays one
  const float vf = (float)(sc * ((double)wmap[b * hw + pix] * sgn));
  dsr[q] = accumulate ? dsr[q] + vf : vf;
}

// ------------------------------------------------------------------------------------------ host
static int artifact_check(const char* who, int B, int H, int W, int ksize) {
  SST_REQUIRE(ksize >= 3 && ksize <= AMAXK && (ksize & 1), "%s: ksize must be odd, 3..%d, got %d", who, AMAXK, ksize);
  SST_REQUIRE(B > 0 && B <= 65535, "%s: bad batch %d", who, B);
  const int p = ksize / 2;
  SST_REQUIRE(H >= p + 1 && W >= p + 1, "%s: image %dx%d is below the %d-px minimum of the reflected %dx%d window", who, W, H, p + 1,
              ksize, ksize);
  SST_REQUIRE((H + AT - 1) / AT <= 65535, "%s: bad image size %dx%d", who, W, H);
  SST_REQUIRE((int64_t)B * ((H + AT - 1) / AT) * ((W + AT - 1) / AT) < ((int64_t)1 << 31), "%s: too many tiles", who);
  SST_REQUIRE(((int64_t)B * 3 * H * W + ANT - 1) / ANT < ((int64_t)1 << 31), "%s: too many elements", who);
  return SST_OK;
}

static dim3 artifact_grid(int B, int H, int W) { return dim3((W + AT - 1) / AT, (H + AT - 1) / AT, B); }

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_artifact_loss_workspace(int B, int H, int W, int ksize, int64_t* map_floats, int64_t* stat_floats,
                                        int64_t* partial_floats) {
  SST_REQUIRE(map_floats && stat_floats && partial_floats, "sst_artifact_loss_workspace: null pointer");
  if (int rc = artifact_check("sst_artifact_loss_workspace", B, H, W, ksize)) return rc;
  const dim3 g = artifact_grid(B, H, W);
  const int64_t nblk = (int64_t)g.x * g.y * g.z;
  *map_floats = (int64_t)B * H * W;                            // w, one float per pixel
  *stat_floats = 2 * (2 * nblk + B);                           // fp64: S1 and S2 per workgroup, then the B global weights
  *partial_floats = 2 * nblk;                                  // one fp64 partial per workgroup
  return SST_OK;
}

SST_API int sst_artifact_loss_fwd(const float* sr, const float* gt, const float* ref, float* loss, float* wmap, float* stats,
                                  unsigned* stat_counter, float* partials, unsigned* counter, int B, int H, int W, int ksize,
                                  void* stream) {
  SST_REQUIRE(sr && gt && loss && stats && stat_counter && partials && counter, "sst_artifact_loss_fwd: null pointer");
  SST_REQUIRE(((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(stats)) & 7) == 0,
              "sst_artifact_loss_fwd: stats and partials must be 8-byte aligned");
  if (int rc = artifact_check("sst_artifact_loss_fwd", B, H, W, ksize)) return rc;
  const dim3 grid = artifact_grid(B, H, W);
  const int64_t nblk = (int64_t)grid.x * grid.y * grid.z;
  double* st = reinterpret_cast<double*>(stats);
  double* part = reinterpret_cast<double*>(partials);
  const double count = (double)B * 3.0 * (double)H * (double)W;
  hipStream_t s = sst_stream(stream);
  artifact_stats_kernel<<<grid, ANT, 0, s>>>(sr, gt, st, stat_counter, H, W);
  SST_LAUNCH_CHECK("artifact_stats_kernel");
  const double* weights = st + 2 * nblk;
#define SST_ARTIFACT_FWD(K) \
  artifact_loss_fwd_kernel<K><<<grid, ANT, 0, s>>>(sr, gt, ref, weights, wmap, part, counter, loss, H, W, count)
  switch (ksize) {
    case 3: SST_ARTIFACT_FWD(3); break;
    case 5: SST_ARTIFACT_FWD(5); break;
    case 7: SST_ARTIFACT_FWD(7); break;
    case 9: SST_ARTIFACT_FWD(9); break;
    default: SST_ARTIFACT_FWD(11); break;
  }
#undef SST_ARTIFACT_FWD
  SST_LAUNCH_CHECK("artifact_loss_fwd_kernel");
  return SST_OK;
}

SST_API int sst_artifact_loss_bwd(const float* sr, const float* gt, const float* wmap, float* dsr, const float* scale_dev,
                                  float scale_host, int accumulate, int B, int H, int W, int ksize, void* stream) {
  SST_REQUIRE(sr && gt && wmap && dsr, "sst_artifact_loss_bwd: null pointer");
  if (int rc = artifact_check("sst_artifact_loss_bwd", B, H, W, ksize)) return rc;
  const int64_t hw = (int64_t)H * W, total = (int64_t)B * 3 * hw;
  const double scale = (double)scale_host / ((double)B * 3.0 * (double)H * (double)W);
  artifact_loss_bwd_kernel<<<(unsigned)((total + ANT - 1) / ANT), ANT, 0, sst_stream(stream)>>>(sr, gt, wmap, dsr, scale_dev, scale,
                                                                                                accumulate, hw, total);
  SST_LAUNCH_CHECK("artifact_loss_bwd_kernel");
  return SST_OK;
}
