// The two first-order siblings of the structure-tensor loss (loss.py: GradientLoss, GradientVarianceLoss), forward and backward, for
// gfx950.  "Correlation" is F.conv2d with padding = 1: pixels outside the image count as zero.  The vertical operator responds to
// row-to-row change, the horizontal one is its transpose:
//
//   central (op 0)  Kv = [[0,-1,0],[0,0,0],[0,1,0]]        sobel (op 1)  Kv = [[-1,-2,-1],[0,0,0],[1,2,1]]        Kh = Kv^T
//
// GradientLoss (the pixel-wise gradient loss of structure-preserving SR, Ma et al., CVPR 2020), per image and RGB plane:
//   M(I) = sqrt(Gv(I)^2 + Gh(I)^2 + eps),  loss = mean over B*3*H*W of |M(sr) - M(gt)| (crit 0) or of its square (crit 1)
// GradientVarianceLoss (Abrahamyan et al., 2022), on gray = 0.2989 R + 0.587 G + 0.114 B with the Sobel operator:
//   the two response maps are cut into non-overlapping p x p patches from the top-left corner (H/p by W/p of them; leftover rows and
//   columns belong to no patch), v = the unbiased variance of a patch, loss = mean((vv(sr) - vv(gt))^2) + mean((vh(sr) - vh(gt))^2)
//
// Arithmetic: the staged value (a plane's pixel, or the gray value rounded once) is fp32; everything after it is fp64 - the tap sums
// (exact: a few 24-bit values), the magnitude, the patch mean and the centred sum of squares, every reduction.  sr and gt go through
// the same instructions and meet in a plain difference (M(sr) - M(gt), css(sr) - css(gt)) before anything scales it, so sr == gt is a
// loss of exactly 0 and a gradient of exactly 0 whether or not the compiler fuses multiplies into adds (the library is built with
// -ffp-contract=fast); an accumulating store adds a value already rounded to fp32, so it is the plain store's value plus the prefill.
//
// GradientLoss forward: one workgroup per 32 x 32 tile, plane and image; the tile of sr and gt with a 1-px ring in LDS; one fp64
// partial per workgroup, summed in index order by the last arriver (common.h), which re-arms the counter.  Nothing is saved.
// GradientLoss backward: the same tile with a 2-px ring; (Gv, Gh, M) of both images on the tile plus a 1-px ring, there
//   A = dM G / M(sr),  dM = sign(M(sr) - M(gt)) (0 at a tie) or 2 (M(sr) - M(gt)),  0 outside the image
// as two fp32 planes in LDS; d(sr)[q] gathers its own taps of the adjoint of the zero-padded correlation - no atomics.
//
// GradientVarianceLoss forward: a workgroup owns whole patches - a tile of side p * floor(32 / p) (32 at p = 8, 30 at p = 3 or 5, p
// from 17 on).  Gray of both images with a 1-px ring, the four response maps (fp32) of the tile, then per patch the mean and, in a
// second pass over the LDS tile, the centred sum of squares (never E[x^2] - E[x]^2), each as row sums followed by a sum over the
// patch's rows, in a fixed order.  With saved != null it writes per patch (mean of sr's Gv, d loss / d vv, mean of sr's Gh,
// d loss / d vh).  Backward: gray of sr with a 2-px ring, sr's responses on the tile plus a 1-px ring,
//   dG = (d loss / d v) 2 (G - mean) / (p^2 - 1) inside the patch grid, 0 outside it,
// gathered through the transposed Sobel taps and spread to R, G, B by the gray weights.  gt is not read.
//
// NaN: every comparison that guards a load or a position selects the value or a literal zero, so a NaN in sr reaches the loss and
// d(sr) around it (5 x 5 pixels of its plane; the patches that meet its 3 x 3 neighbourhood, grown by 1 px) - and nothing else.
#include "common.h"

#include <cmath>

namespace {

constexpr int GT = 32;                 // tile edge (GradientVarianceLoss: the largest)
constexpr int GP = GT + 5;             // LDS row pitch of a staged plane (up to GT + 4 columns), odd
constexpr int GNT = 256;
constexpr int GVMAXN = 16;             // patches per tile side at the smallest patch (2)
constexpr int GGP = GT + 1;            // LDS row pitch of a response map of the tile
constexpr double GRAY_R = 0.2989, GRAY_G = 0.587, GRAY_B = 0.114;

// (Gv, Gh) at the staged position c (row pitch GP): sums of a few fp32 values, exact in fp64
template <int OP>
__device__ __forceinline__ void responses(const float* c, double& gv, double& gh) {
  if (OP == 0) {
    gv = (double)c[GP] - (double)c[-GP];
    gh = (double)c[1] - (double)c[-1];
  } else {
    const double tl = c[-GP - 1], tc = c[-GP], tr = c[-GP + 1], l = c[-1], r = c[1], bl = c[GP - 1], bc = c[GP], br = c[GP + 1];
    gv = (bl + 2.0 * bc + br) - (tl + 2.0 * tc + tr);
    gh = (tr + 2.0 * r + br) - (tl + 2.0 * l + bl);
  }
}

// The adjoint of both zero-padded correlations at q, from the planes of d loss / d Gv and d loss / d Gh (row pitch GP, zero outside
// the image): position q - o received tap K[o], so q sums K[o] * A[q - o]
template <int OP>
__device__ __forceinline__ double adjoint(const float* av, const float* ah) {
  if (OP == 0) return ((double)av[-GP] - (double)av[GP]) + ((double)ah[-1] - (double)ah[1]);
  const double v = ((double)av[-GP - 1] + 2.0 * (double)av[-GP] + (double)av[-GP + 1]) -
                   ((double)av[GP - 1] + 2.0 * (double)av[GP] + (double)av[GP + 1]);
  const double h = ((double)ah[-GP - 1] + 2.0 * (double)ah[-1] + (double)ah[GP - 1]) -
                   ((double)ah[-GP + 1] + 2.0 * (double)ah[1] + (double)ah[GP + 1]);
  return v + h;
}

__device__ __forceinline__ float gray_value(const float* __restrict__ img, int64_t hw, int64_t o) {
  return (float)(((double)img[o] * GRAY_R + (double)img[o + hw] * GRAY_G) + (double)img[o + 2 * hw] * GRAY_B);
}

// Stages side x side values with origin (y0, x0) into s (row pitch GP): the plane's pixel, or the gray value of the three planes
// hw apart; zero outside the image
template <bool GRAY>
__device__ __forceinline__ void stage(float* s, const float* __restrict__ img, int H, int W, int y0, int x0, int side) {
  const int64_t hw = (int64_t)H * W;
  for (int i = threadIdx.x; i < side * side; i += GNT) {
    const int r = i / side, c = i - r * side;
    const int gy = y0 + r, gx = x0 + c;
    float v = 0.f;
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
      const int64_t o = (int64_t)gy * W + gx;
      v = GRAY ? gray_value(img, hw, o) : img[o];
    }
    s[r * GP + c] = v;
  }
}

// -------------------------------------------------------------------------------------------- GradientLoss
template <int OP>
__global__ __launch_bounds__(GNT) void grad_loss_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt, double* partials,
                                                            unsigned* counter, float* __restrict__ loss, int H, int W, int crit,
                                                            double eps, double count) {
  __shared__ float s_x[(GT + 2) * GP], s_y[(GT + 2) * GP];
  __shared__ double s_red[GNT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * GT, y0 = blockIdx.y * GT;
  const int64_t img = (int64_t)blockIdx.z * H * W;            // z = image * 3 + plane
  stage<false>(s_x, sr + img, H, W, y0 - 1, x0 - 1, GT + 2);
  stage<false>(s_y, gt + img, H, W, y0 - 1, x0 - 1, GT + 2);
  __syncthreads();

  double ss = 0.0;
  for (int i = tid; i < GT * GT; i += GNT) {
    const int j = i / GT, c = i % GT;
    if (y0 + j < H && x0 + c < W) {
      const int o = (j + 1) * GP + c + 1;
      double gvx, ghx, gvy, ghy;
      responses<OP>(s_x + o, gvx, ghx);
      responses<OP>(s_y + o, gvy, ghy);
      const double d = sqrt(gvx * gvx + ghx * ghx + eps) - sqrt(gvy * gvy + ghy * ghy + eps);
      ss += crit ? d * d : fabs(d);
    }
  }
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const unsigned blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (!last_block_arrive_d<GNT>(ss, partials, blk, counter, nblk, &s_flag, s_red)) return;
  const double t = last_block_total_d<GNT>(partials, counter, nblk, s_red);
  if (tid == 0) loss[0] = (float)(t / count);
}

// dsr (+)= scale * (scale_dev ? *scale_dev : 1) * (the adjoint of the two correlations on dM G / M);  scale = scale_host / count
template <int OP>
__global__ __launch_bounds__(GNT) void grad_loss_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                            float* __restrict__ dsr, const float* __restrict__ scale_dev, double scale,
                                                            int accumulate, int H, int W, int crit, double eps) {
  __shared__ float s_x[(GT + 4) * GP], s_y[(GT + 4) * GP];
  __shared__ float s_av[(GT + 2) * GP], s_ah[(GT + 2) * GP];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * GT, y0 = blockIdx.y * GT;
  const int64_t img = (int64_t)blockIdx.z * H * W;
  stage<false>(s_x, sr + img, H, W, y0 - 2, x0 - 2, GT + 4);
  stage<false>(s_y, gt + img, H, W, y0 - 2, x0 - 2, GT + 4);
  __syncthreads();
  // ---- A = dM G / M(sr) on the tile plus a 1-px ring; zero outside the image
  for (int i = tid; i < (GT + 2) * (GT + 2); i += GNT) {
    const int r = i / (GT + 2), c = i - r * (GT + 2);
    const int py = y0 - 1 + r, px = x0 - 1 + c;
    float av = 0.f, ah = 0.f;
    if ((unsigned)py < (unsigned)H && (unsigned)px < (unsigned)W) {
      const int o = (r + 1) * GP + c + 1;
      double gvx, ghx, gvy, ghy;
      responses<OP>(s_x + o, gvx, ghx);
      responses<OP>(s_y + o, gvy, ghy);
      const double mx = sqrt(gvx * gvx + ghx * ghx + eps);
      const double d = mx - sqrt(gvy * gvy + ghy * ghy + eps);
      const double dm = crit ? 2.0 * d : (d > 0.0 ? 1.0 : d < 0.0 ? -1.0 : d);      // a tie gives 0, a NaN stays one
      const double k = dm / mx;
      av = (float)(k * gvx);
      ah = (float)(k * ghx);
    }
    s_av[r * GP + c] = av;
    s_ah[r * GP + c] = ah;
  }
  __syncthreads();
  double sc = scale;
  if (scale_dev) sc = sc * (double)scale_dev[0];
  for (int i = tid; i < GT * GT; i += GNT) {
    const int j = i / GT, c = i % GT;
    const int qy = y0 + j, qx = x0 + c;
    if (qy >= H || qx >= W) continue;
    const int o = (j + 1) * GP + c + 1;
    const float vf = (float)(adjoint<OP>(s_av + o, s_ah + o) * sc);
    const int64_t q = img + (int64_t)qy * W + qx;
    dsr[q] = accumulate ? dsr[q] + vf : vf;
  }
}

// -------------------------------------------------------------------------------------------- GradientVarianceLoss
// The four response maps are numbered q = image * 2 + direction (image 0 = sr, direction 0 = vertical).
__global__ __launch_bounds__(GNT) void gv_loss_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                          float* __restrict__ saved, double* partials, unsigned* counter,
                                                          float* __restrict__ loss, int H, int W, int p, int PH, int PW, double npatch) {
  __shared__ float s_gray[2][(GT + 2) * GP];
  __shared__ float s_g[4][GT * GGP];
  __shared__ double s_row[4][GT][GVMAXN];          // per map, tile row and patch column: a row sum
  __shared__ double s_mean[4][GVMAXN * GVMAXN];
  __shared__ double s_red[GNT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x, b = blockIdx.z;
  const int n = GT / p, ts = n * p;                // patches per tile side, tile side
  const int x0 = blockIdx.x * ts, y0 = blockIdx.y * ts;
  const int nvr = min(n, PH - (int)blockIdx.y * n), nvc = min(n, PW - (int)blockIdx.x * n);      // the patches this tile really has
  const int rows = nvr * p, cols = nvc * p;
  const int64_t img = (int64_t)b * 3 * H * W;
  stage<true>(s_gray[0], sr + img, H, W, y0 - 1, x0 - 1, ts + 2);
  stage<true>(s_gray[1], gt + img, H, W, y0 - 1, x0 - 1, ts + 2);
  __syncthreads();
  // ---- the four response maps on the tile's patches
  for (int i = tid; i < ts * ts; i += GNT) {
    const int j = i / ts, c = i - j * ts;
    if (j < rows && c < cols) {
      const int o = (j + 1) * GP + c + 1;
      double gv, gh;
      responses<1>(s_gray[0] + o, gv, gh);
      s_g[0][j * GGP + c] = (float)gv;
      s_g[1][j * GGP + c] = (float)gh;
      responses<1>(s_gray[1] + o, gv, gh);
      s_g[2][j * GGP + c] = (float)gv;
      s_g[3][j * GGP + c] = (float)gh;
    }
  }
  __syncthreads();
  const double inv_pp = 1.0 / (double)(p * p), inv_nm1 = 1.0 / (double)(p * p - 1);
  for (int pass = 0; pass < 2; ++pass) {
    // ---- row sums per patch column: of the responses, then of their squared distance to the patch mean
    for (int t = tid; t < 4 * ts * n; t += GNT) {
      const int q = t / (ts * n), rem = t - q * (ts * n);
      const int r = rem / n, pc = rem - r * n;
      if (r < rows && pc < nvc) {
        const float* g = s_g[q] + r * GGP + pc * p;
        double s = 0.0;
        if (pass == 0) {
          for (int k = 0; k < p; ++k) s += (double)g[k];
        } else {
          const double m = s_mean[q][(r / p) * GVMAXN + pc];
          for (int k = 0; k < p; ++k) {
            const double e = (double)g[k] - m;
            s += e * e;
          }
        }
        s_row[q][r][pc] = s;
      }
    }
    __syncthreads();
    if (pass == 1) break;
    // ---- patch means
    for (int t = tid; t < 4 * n * n; t += GNT) {
      const int q = t / (n * n), rem = t - q * (n * n);
      const int pr = rem / n, pc = rem - pr * n;
      if (pr < nvr && pc < nvc) {
        double s = 0.0;
        for (int k = 0; k < p; ++k) s += s_row[q][pr * p + k][pc];
        s_mean[q][pr * GVMAXN + pc] = s * inv_pp;
      }
    }
    __syncthreads();
  }
  // ---- variances, their squared differences, and what the backward reads
  double ss = 0.0;
  for (int t = tid; t < 2 * n * n; t += GNT) {
    const int dir = t / (n * n), rem = t - dir * (n * n);
    const int pr = rem / n, pc = rem - pr * n;
    if (pr < nvr && pc < nvc) {
      double cx = 0.0, cy = 0.0;
      for (int k = 0; k < p; ++k) {
        cx += s_row[dir][pr * p + k][pc];
        cy += s_row[2 + dir][pr * p + k][pc];
      }
      const double d = (cx - cy) * inv_nm1;          // the difference first: equal sums give 0 whatever the compiler fuses
      ss += d * d;
      if (saved) {
        const int64_t o = ((((int64_t)b * PH + (blockIdx.y * n + pr)) * PW + (blockIdx.x * n + pc)) * 2 + dir) * 2;
        saved[o] = (float)s_mean[dir][pr * GVMAXN + pc];
        saved[o + 1] = (float)(2.0 * d / npatch);
      }
    }
  }
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const unsigned blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (!last_block_arrive_d<GNT>(ss, partials, blk, counter, nblk, &s_flag, s_red)) return;
  const double t = last_block_total_d<GNT>(partials, counter, nblk, s_red);
  if (tid == 0) loss[0] = (float)(t / npatch);
}

// dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * gray weight * (the adjoint of the two Sobel correlations on dG)
__global__ __launch_bounds__(GNT) void gv_loss_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ saved,
                                                          float* __restrict__ dsr, const float* __restrict__ scale_dev, double scale,
                                                          int accumulate, int H, int W, int p, int PH, int PW) {
  __shared__ float s_gray[(GT + 4) * GP];
  __shared__ float s_dv[(GT + 2) * GP], s_dh[(GT + 2) * GP];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int ts = (GT / p) * p;
  const int x0 = blockIdx.x * ts, y0 = blockIdx.y * ts;
  const int64_t hw = (int64_t)H * W, img = (int64_t)b * 3 * hw;
  stage<true>(s_gray, sr + img, H, W, y0 - 2, x0 - 2, ts + 4);
  __syncthreads();
  // ---- dG on the tile plus a 1-px ring; zero outside the patch grid
  const double k2 = 2.0 / (double)(p * p - 1);
  const int gh_ = PH * p, gw_ = PW * p;                        // the patch grid's extent
  for (int i = tid; i < (ts + 2) * (ts + 2); i += GNT) {
    const int r = i / (ts + 2), c = i - r * (ts + 2);
    const int py = y0 - 1 + r, px = x0 - 1 + c;
    float dv = 0.f, dh = 0.f;
    if ((unsigned)py < (unsigned)gh_ && (unsigned)px < (unsigned)gw_) {
      const float* st = saved + (((int64_t)b * PH + py / p) * PW + px / p) * 4;
      double gv, gh;
      responses<1>(s_gray + (r + 1) * GP + c + 1, gv, gh);
      dv = (float)((double)st[1] * (k2 * (gv - (double)st[0])));
      dh = (float)((double)st[3] * (k2 * (gh - (double)st[2])));
    }
    s_dv[r * GP + c] = dv;
    s_dh[r * GP + c] = dh;
  }
  __syncthreads();
  double sc = scale;
  if (scale_dev) sc = sc * (double)scale_dev[0];
  for (int i = tid; i < ts * ts; i += GNT) {
    const int j = i / ts, c = i - j * ts;
    const int qy = y0 + j, qx = x0 + c;
    if (qy >= H || qx >= W) continue;
    const int o = (j + 1) * GP + c + 1;
    const double v = adjoint<1>(s_dv + o, s_dh + o) * sc;
    const float vr = (float)(v * GRAY_R), vg = (float)(v * GRAY_G), vb = (float)(v * GRAY_B);
    const int64_t q = img + (int64_t)qy * W + qx;
    if (accumulate) {
      dsr[q] = dsr[q] + vr;
      dsr[q + hw] = dsr[q + hw] + vg;
      dsr[q + 2 * hw] = dsr[q + 2 * hw] + vb;
    } else {
      dsr[q] = vr;
      dsr[q + hw] = vg;
      dsr[q + 2 * hw] = vb;
    }
  }
}

// ------------------------------------------------------------------------------------------ host
static int grad_check(const char* who, int B, int H, int W, int op, int crit, double eps) {
  SST_REQUIRE(B > 0 && (int64_t)B * 3 <= 65535, "%s: bad batch %d", who, B);
  SST_REQUIRE(H > 0 && W > 0 && (H + GT - 1) / GT <= 65535, "%s: bad image size %dx%d", who, W, H);
  SST_REQUIRE((int64_t)B * 3 * ((H + GT - 1) / GT) * ((W + GT - 1) / GT) < ((int64_t)1 << 31), "%s: too many tiles", who);
  SST_REQUIRE(op == 0 || op == 1, "%s: op must be 0 (central) or 1 (sobel), got %d", who, op);
  SST_REQUIRE(crit == 0 || crit == 1, "%s: crit must be 0 (l1) or 1 (mse), got %d", who, crit);
  SST_REQUIRE(eps > 0.0 && std::isfinite(eps), "%s: eps must be finite and positive, got %g", who, eps);
  return SST_OK;
}

static int gv_check(const char* who, int B, int H, int W, int patch) {
  SST_REQUIRE(patch >= 2 && patch <= GT, "%s: patch must be 2..%d, got %d", who, GT, patch);
  SST_REQUIRE(B > 0 && B <= 65535, "%s: bad batch %d", who, B);
  SST_REQUIRE(H >= patch && W >= patch, "%s: image %dx%d is below the patch size %d", who, W, H, patch);
  const int ts = (GT / patch) * patch;
  SST_REQUIRE((H + ts - 1) / ts <= 65535, "%s: bad image size %dx%d", who, W, H);
  SST_REQUIRE((int64_t)B * ((H + ts - 1) / ts) * ((W + ts - 1) / ts) < ((int64_t)1 << 31), "%s: too many tiles", who);
  return SST_OK;
}

static dim3 grad_grid(int B, int H, int W) { return dim3((W + GT - 1) / GT, (H + GT - 1) / GT, B * 3); }

// the forward's grid: the tiles that hold a patch
static dim3 gv_fwd_grid(int B, int H, int W, int patch) {
  const int n = GT / patch;
  return dim3((W / patch + n - 1) / n, (H / patch + n - 1) / n, B);
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_grad_loss_workspace(int B, int H, int W, int64_t* partial_floats) {
  SST_REQUIRE(partial_floats, "sst_grad_loss_workspace: null pointer");
  if (int rc = grad_check("sst_grad_loss_workspace", B, H, W, 0, 0, 1.0)) return rc;
  const dim3 g = grad_grid(B, H, W);
  *partial_floats = 2 * (int64_t)g.x * g.y * g.z;                        // one fp64 partial per workgroup
  return SST_OK;
}

SST_API int sst_grad_loss_fwd(const float* sr, const float* gt, float* loss, float* partials, unsigned* counter, int B, int H, int W,
                              int op, int crit, double eps, void* stream) {
  SST_REQUIRE(sr && gt && loss && partials && counter, "sst_grad_loss_fwd: null pointer");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "sst_grad_loss_fwd: partials must be 8-byte aligned");
  if (int rc = grad_check("sst_grad_loss_fwd", B, H, W, op, crit, eps)) return rc;
  const double count = (double)B * 3.0 * (double)H * (double)W;
  double* part = reinterpret_cast<double*>(partials);
  if (op == 0)
    grad_loss_fwd_kernel<0><<<grad_grid(B, H, W), GNT, 0, sst_stream(stream)>>>(sr, gt, part, counter, loss, H, W, crit, eps, count);
  else
    grad_loss_fwd_kernel<1><<<grad_grid(B, H, W), GNT, 0, sst_stream(stream)>>>(sr, gt, part, counter, loss, H, W, crit, eps, count);
  SST_LAUNCH_CHECK("grad_loss_fwd_kernel");
  return SST_OK;
}

SST_API int sst_grad_loss_bwd(const float* sr, const float* gt, float* dsr, const float* scale_dev, float scale_host, int accumulate,
                              int B, int H, int W, int op, int crit, double eps, void* stream) {
  SST_REQUIRE(sr && gt && dsr, "sst_grad_loss_bwd: null pointer");
  if (int rc = grad_check("sst_grad_loss_bwd", B, H, W, op, crit, eps)) return rc;
  const double scale = (double)scale_host / ((double)B * 3.0 * (double)H * (double)W);
  if (op == 0)
    grad_loss_bwd_kernel<0><<<grad_grid(B, H, W), GNT, 0, sst_stream(stream)>>>(sr, gt, dsr, scale_dev, scale, accumulate, H, W, crit, eps);
  else
    grad_loss_bwd_kernel<1><<<grad_grid(B, H, W), GNT, 0, sst_stream(stream)>>>(sr, gt, dsr, scale_dev, scale, accumulate, H, W, crit, eps);
  SST_LAUNCH_CHECK("grad_loss_bwd_kernel");
  return SST_OK;
}

SST_API int sst_gv_loss_workspace(int B, int H, int W, int patch, int64_t* saved_floats, int64_t* partial_floats) {
  SST_REQUIRE(saved_floats && partial_floats, "sst_gv_loss_workspace: null pointer");
  if (int rc = gv_check("sst_gv_loss_workspace", B, H, W, patch)) return rc;
  const dim3 g = gv_fwd_grid(B, H, W, patch);
  *saved_floats = 4 * (int64_t)B * (H / patch) * (W / patch);
  *partial_floats = 2 * (int64_t)g.x * g.y * g.z;                        // one fp64 partial per workgroup
  return SST_OK;
}

SST_API int sst_gv_loss_fwd(const float* sr, const float* gt, float* loss, float* saved, float* partials, unsigned* counter, int B,
                            int H, int W, int patch, void* stream) {
  SST_REQUIRE(sr && gt && loss && partials && counter, "sst_gv_loss_fwd: null pointer");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "sst_gv_loss_fwd: partials must be 8-byte aligned");
  if (int rc = gv_check("sst_gv_loss_fwd", B, H, W, patch)) return rc;
  const int PH = H / patch, PW = W / patch;
  gv_loss_fwd_kernel<<<gv_fwd_grid(B, H, W, patch), GNT, 0, sst_stream(stream)>>>(sr, gt, saved, reinterpret_cast<double*>(partials),
                                                                                 counter, loss, H, W, patch, PH, PW,
                                                                                 (double)B * (double)PH * (double)PW);
  SST_LAUNCH_CHECK("gv_loss_fwd_kernel");
  return SST_OK;
}

SST_API int sst_gv_loss_bwd(const float* sr, const float* saved, float* dsr, const float* scale_dev, float scale_host, int accumulate,
                            int B, int H, int W, int patch, void* stream) {
  SST_REQUIRE(sr && saved && dsr, "sst_gv_loss_bwd: null pointer");
  if (int rc = gv_check("sst_gv_loss_bwd", B, H, W, patch)) return rc;
  const int ts = (GT / patch) * patch;
  const dim3 grid((W + ts - 1) / ts, (H + ts - 1) / ts, B);               // every pixel of d(sr), leftover rows and columns included
  gv_loss_bwd_kernel<<<grid, GNT, 0, sst_stream(stream)>>>(sr, saved, dsr, scale_dev, (double)scale_host, accumulate, H, W, patch,
                                                          H / patch, W / patch);
  SST_LAUNCH_CHECK("gv_loss_bwd_kernel");
  return SST_OK;
}
