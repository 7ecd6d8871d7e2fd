// SSIM loss (loss.py: SSIMLoss), forward and backward, for gfx950: loss = 1 - mean(S) over batch, planes and the (H-10) x (W-10)
// valid region of the 11-tap sigma 1.5 Gaussian window - the SSIM validate reports (metrics.hip), as a differentiable criterion.
//
//   planes = 1 ("y"):   P = (65.481 R + 128.553 G + 24.966 B + 16) / 255      (no quantisation, no clamp)
//   planes = 3 ("rgb"): the three input planes as they are
//   a = w (*) x, b = w (*) y, exx = w (*) x^2, eyy = w (*) y^2, exy = w (*) xy      separable, 'valid'; x from sr, y from gt
//   N1 = 2ab + C1, N2 = 2(exy - ab) + C2, D1 = a^2 + b^2 + C1, D2 = (exx - a^2) + (eyy - b^2) + C2, S = N1 N2 / (D1 D2)
//
// Everything after the load is fp64 (the window sums, exx - a^2, the quotient, every reduction): the plane value is rounded to
// fp32 once, so x*x, y*y and x*y are exact in fp64.  This file turns contraction off and spells fma() out where fusing is wanted.
//
// Forward: one workgroup per 32 x 32 tile of outputs, plane and image (grid z = image * planes + plane).  Output (oy, ox) reads
// inputs [oy, oy+10] x [ox, ox+10]: the workgroup stages the tile plus the 10-px apron to the right and below as two fp32 planes in
// LDS, then per half tile of 16 output rows a horizontal pass of the five quantities into LDS (26 rows) and a vertical pass with the
// quotient.  With maps != null it also writes the three maps the backward filters, fp32 [B*planes][3][H-10][W-10]:
//   Ga  = dS/da   = 2b (N2 - N1) / (D1 D2) - 2a S (D2 - D1) / (D1 D2)        (exx, eyy, exy held fixed)
//   Gxx = dS/dexx = -S / D2
//   Gxy = dS/dexy = 2 N1 / (D1 D2)
// - no division by N1 or N2 (N2 <= 0 where sr and gt anti-correlate).  One fp64 partial per workgroup; the last-arriving workgroup
// sums the partials in index order and re-arms the counter: no floating-point atomics, the same bits in every run and replay.
//
// Backward: one workgroup per 32 x 32 tile of sr pixels, plane and image.  Pixel q collects from the outputs [q-10, q]: the three
// maps with a 10-px apron to the left and above (zero outside the valid region) go to LDS, a horizontal and a vertical pass give the
// three full correlations, and
//   dP[q] = -scale / (B planes (H-10)(W-10)) * ( (w (*)T Ga)[q] + 2 x[q] (w (*)T Gxx)[q] + y[q] (w (*)T Gxy)[q] )
// is stored (or added) to the plane's channel, or spread to R, G, B by the luma coefficients.
//
// NaN: every comparison that guards a load selects the loaded value or a literal zero, so a NaN in sr reaches S of every window
// that holds it, the loss, and dsr around it - and nothing else.
#include "common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int LT = 32;                 // tile edge
constexpr int LK = 11;                 // Gaussian taps
constexpr int LA = LK - 1;             // apron: 10
constexpr int LS = LT + LA;            // staged edge: 42
constexpr int LSP = LS + 1;            // LDS row pitch of the staged fp32 planes
constexpr int LHALF = 16;              // forward: output rows per half tile
constexpr int LHR = LHALF + LA;        // forward: horizontal-pass rows per half tile: 26
constexpr int LNT = 256;

struct SsimTaps {
  double w[LK];
};

// utils._gaussian_window's 1-D factor, normalised in fp64 (the sum taken as numpy's pairwise add takes 11 terms): metrics.hip's taps
static SsimTaps ssim_taps() {
  SsimTaps t;
  const double sigma = 1.5;
  for (int i = 0; i < LK; ++i) {
    const double x = (double)i - (LK - 1) / 2.0;
    t.w[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
  }
  double s = ((t.w[0] + t.w[1]) + (t.w[2] + t.w[3])) + ((t.w[4] + t.w[5]) + (t.w[6] + t.w[7]));
  for (int i = 8; i < LK; ++i) s += t.w[i];
  for (int i = 0; i < LK; ++i) t.w[i] /= s;
  return t;
}

constexpr double LUMA_R = 65.481, LUMA_G = 128.553, LUMA_B = 24.966;

// the plane value at offset o: planes == 1 -> luma of the three channels at img (hw apart), else the channel at img itself
__device__ __forceinline__ float plane_value(const float* __restrict__ img, int64_t hw, int64_t o, int planes) {
  if (planes != 1) return img[o];
  const double r = (double)img[o], g = (double)img[o + hw], b = (double)img[o + 2 * hw];
  return (float)((((r * LUMA_R + g * LUMA_G) + b * LUMA_B) + 16.0) / 255.0);
}

__global__ __launch_bounds__(LNT) void ssim_loss_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                            float* __restrict__ maps, double* partials, unsigned* counter,
                                                            float* __restrict__ loss, int H, int W, int planes, double C1, double C2,
                                                            double count, SsimTaps taps) {
  __shared__ float s_x[LS * LSP], s_y[LS * LSP];
  __shared__ double s_h[5][LHR][LT];
  __shared__ double s_red[LNT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x, z = blockIdx.z, b = z / planes, p = z - b * planes;
  const int ox0 = blockIdx.x * LT, oy0 = blockIdx.y * LT;
  const int Ho = H - LA, Wo = W - LA;
  const int64_t hw = (int64_t)H * W, howo = (int64_t)Ho * Wo;
  const int64_t img = ((int64_t)b * 3 + (planes == 1 ? 0 : p)) * hw;
  const float* xb = sr + img;
  const float* yb = gt + img;

  // ---- stage the tile and its apron, one plane value per pixel
  for (int i = tid; i < LS * LS; i += LNT) {
    const int r = i / LS, c = i - r * LS;
    const int gy = oy0 + r, gx = ox0 + c;
    float xs = 0.f, ys = 0.f;
    if (gy < H && gx < W) {
      const int64_t o = (int64_t)gy * W + gx;
      xs = plane_value(xb, hw, o, planes);
      ys = plane_value(yb, hw, o, planes);
    }
    s_x[r * LSP + c] = xs;
    s_y[r * LSP + c] = ys;
  }
  __syncthreads();

  double ss = 0.0;
  for (int half = 0; half < LT / LHALF; ++half) {
    // ---- horizontal pass: rows [16*half, 16*half + 26) of the staged planes, 32 columns, five quantities
    for (int i = tid; i < LHR * LT; i += LNT) {
      const int rr = i / LT, c = i % LT;
      const float* px = s_x + (half * LHALF + rr) * LSP + c;
      const float* py = s_y + (half * LHALF + rr) * LSP + c;
      double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
      for (int t = 0; t < LK; ++t) {
        const double w = taps.w[t], x = (double)px[t], y = (double)py[t];
        ax = fma(w, x, ax);
        ay = fma(w, y, ay);
        axx = fma(w, x * x, axx);          // x*x, y*y, x*y are exact in fp64 (24-bit factors)
        ayy = fma(w, y * y, ayy);
        axy = fma(w, x * y, axy);
      }
      s_h[0][rr][c] = ax;
      s_h[1][rr][c] = ay;
      s_h[2][rr][c] = axx;
      s_h[3][rr][c] = ayy;
      s_h[4][rr][c] = axy;
    }
    __syncthreads();
    // ---- vertical pass, quotient and the three maps: 16 x 32 outputs, two per thread
    for (int i = tid; i < LHALF * LT; i += LNT) {
      const int j = i / LT, c = i % LT;
      const int oy = oy0 + half * LHALF + j, ox = ox0 + c;
      if (oy < Ho && ox < Wo) {
        double a = 0.0, bm = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
        for (int t = 0; t < LK; ++t) {
          const double w = taps.w[t];
          a = fma(w, s_h[0][j + t][c], a);
          bm = fma(w, s_h[1][j + t][c], bm);
          exx = fma(w, s_h[2][j + t][c], exx);
          eyy = fma(w, s_h[3][j + t][c], eyy);
          exy = fma(w, s_h[4][j + t][c], exy);
        }
        const double aa = a * a, bb = bm * bm, ab = a * bm;
        const double N1 = 2.0 * ab + C1, N2 = 2.0 * (exy - ab) + C2;
        const double D1 = aa + bb + C1, D2 = (exx - aa) + (eyy - bb) + C2;
        const double S = (N1 * N2) / (D1 * D2);
        ss += S;
        if (maps) {
          const double iD = 1.0 / (D1 * D2);
          const double ga = 2.0 * bm * (N2 - N1) * iD - 2.0 * a * S * (D2 - D1) * iD;
          const int64_t o = (int64_t)z * 3 * howo + (int64_t)oy * Wo + ox;
          maps[o] = (float)ga;
          maps[o + howo] = (float)(-S / D2);
          maps[o + 2 * howo] = (float)(2.0 * N1 * iD);
        }
      }
    }
    __syncthreads();
  }

  // ---- one partial per workgroup; the last arriver sums them in index order and re-arms the counter
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const unsigned blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (!last_block_arrive_d<LNT>(ss, partials, blk, counter, nblk, &s_flag, s_red)) return;
  const double t = last_block_total_d<LNT>(partials, counter, nblk, s_red);
  if (tid == 0) loss[0] = (float)(1.0 - t / count);
}

// dsr (+)= scale * (scale_dev ? *scale_dev : 1) * (the three full correlations combined);  scale = -scale_host / count
__global__ __launch_bounds__(LNT) void ssim_loss_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                            const float* __restrict__ maps, float* __restrict__ dsr,
                                                            const float* __restrict__ scale_dev, double scale, int accumulate, int H,
                                                            int W, int planes, SsimTaps taps) {
  __shared__ float s_m[3][LS * LSP];
  __shared__ double s_h[3][LS][LT];
  const int tid = threadIdx.x, z = blockIdx.z, b = z / planes, p = z - b * planes;
  const int qx0 = blockIdx.x * LT, qy0 = blockIdx.y * LT;
  const int Ho = H - LA, Wo = W - LA;
  const int64_t hw = (int64_t)H * W, howo = (int64_t)Ho * Wo;
  const float* mb = maps + (int64_t)z * 3 * howo;

  // ---- stage the maps at outputs [q0 - 10, q0 + 32): zero outside the valid region
  for (int i = tid; i < LS * LS; i += LNT) {
    const int r = i / LS, c = i - r * LS;
    const int oy = qy0 - LA + r, ox = qx0 - LA + c;
    const bool in = (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo;
    const int64_t o = (int64_t)oy * Wo + ox;
#pragma unroll
    for (int m = 0; m < 3; ++m) s_m[m][r * LSP + c] = in ? mb[m * howo + o] : 0.f;
  }
  __syncthreads();
  // ---- along W: pixel column c collects from output columns c - t (staged column c + 10 - t)
  for (int i = tid; i < LS * LT; i += LNT) {
    const int r = i / LT, c = i % LT;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const float* pm = s_m[m] + r * LSP + c;
      double h = 0.0;
#pragma unroll
      for (int t = 0; t < LK; ++t) h = fma(taps.w[t], (double)pm[LA - t], h);
      s_h[m][r][c] = h;
    }
  }
  __syncthreads();
  // ---- along H, then the combination with x[q], y[q]
  double sc = scale;
  if (scale_dev) sc = sc * (double)scale_dev[0];
  const int64_t img = ((int64_t)b * 3 + (planes == 1 ? 0 : p)) * hw;
  for (int i = tid; i < LT * LT; i += LNT) {
    const int j = i / LT, c = i % LT;
    const int qy = qy0 + j, qx = qx0 + c;
    if (qy >= H || qx >= W) continue;
    double va = 0.0, vxx = 0.0, vxy = 0.0;
#pragma unroll
    for (int t = 0; t < LK; ++t) {
      const double w = taps.w[t];
      va = fma(w, s_h[0][j + LA - t][c], va);
      vxx = fma(w, s_h[1][j + LA - t][c], vxx);
      vxy = fma(w, s_h[2][j + LA - t][c], vxy);
    }
    const int64_t q = (int64_t)qy * W + qx, o = img + q;
    const double x = (double)plane_value(sr + img, hw, q, planes), y = (double)plane_value(gt + img, hw, q, planes);
    const double v = (va + 2.0 * x * vxx + y * vxy) * sc;
    if (planes == 1) {
      const float vr = (float)(v * (LUMA_R / 255.0)), vg = (float)(v * (LUMA_G / 255.0)), vb = (float)(v * (LUMA_B / 255.0));
      if (accumulate) {
        dsr[o] = dsr[o] + vr;
        dsr[o + hw] = dsr[o + hw] + vg;
        dsr[o + 2 * hw] = dsr[o + 2 * hw] + vb;
      } else {
        dsr[o] = vr;
        dsr[o + hw] = vg;
        dsr[o + 2 * hw] = vb;
      }
    } else {
      const float vf = (float)v;
      dsr[o] = accumulate ? dsr[o] + vf : vf;
    }
  }
}

// shape rules shared by the three entries
static int ssim_check_shape(const char* who, int B, int H, int W, int planes) {
  SST_REQUIRE(planes == 1 || planes == 3, "%s: planes must be 1 (y) or 3 (rgb), got %d", who, planes);
  SST_REQUIRE(B > 0 && (int64_t)B * planes <= 65535, "%s: bad batch %d", who, B);
  SST_REQUIRE(H >= LK && W >= LK, "%s: image %dx%d is below the 11-px minimum of the SSIM window", who, W, H);
  SST_REQUIRE((H + LT - 1) / LT <= 65535, "%s: image height %d needs more than 65535 tile rows", who, H);
  return SST_OK;
}

static int64_t ssim_tiles(int H, int W) { return (int64_t)((H - LA + LT - 1) / LT) * ((W - LA + LT - 1) / LT); }

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_ssim_loss_workspace(int B, int H, int W, int planes, int64_t* map_floats, int64_t* partial_floats) {
  SST_REQUIRE(map_floats && partial_floats, "sst_ssim_loss_workspace: null pointer");
  if (int rc = ssim_check_shape("sst_ssim_loss_workspace", B, H, W, planes)) return rc;
  *map_floats = (int64_t)B * planes * (H - LA) * (int64_t)(W - LA) * 3;
  *partial_floats = 2 * (int64_t)B * planes * ssim_tiles(H, W);          // one fp64 partial per workgroup
  return SST_OK;
}

SST_API int sst_ssim_loss_fwd(const float* sr, const float* gt, float* loss, float* maps, float* partials, unsigned* counter, int B,
                              int H, int W, int planes, double k1, double k2, void* stream) {
  SST_REQUIRE(sr && gt && loss && partials && counter, "sst_ssim_loss_fwd: null pointer");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "sst_ssim_loss_fwd: partials must be 8-byte aligned");
  if (int rc = ssim_check_shape("sst_ssim_loss_fwd", B, H, W, planes)) return rc;
  SST_REQUIRE(k1 > 0.0 && k2 > 0.0 && std::isfinite(k1) && std::isfinite(k2), "sst_ssim_loss_fwd: k1 and k2 must be positive, got %g, %g",
              k1, k2);
  const int Ho = H - LA, Wo = W - LA;
  dim3 grid((Wo + LT - 1) / LT, (Ho + LT - 1) / LT, B * planes);
  SST_REQUIRE((int64_t)grid.x * grid.y * grid.z < ((int64_t)1 << 31), "sst_ssim_loss_fwd: too many tiles");
  const double count = (double)B * planes * (double)Ho * (double)Wo;
  ssim_loss_fwd_kernel<<<grid, LNT, 0, sst_stream(stream)>>>(sr, gt, maps, reinterpret_cast<double*>(partials), counter, loss, H, W,
                                                             planes, k1 * k1, k2 * k2, count, ssim_taps());
  SST_LAUNCH_CHECK("ssim_loss_fwd_kernel");
  return SST_OK;
}

SST_API int sst_ssim_loss_bwd(const float* sr, const float* gt, const float* maps, float* dsr, const float* scale_dev, float scale_host,
                              int accumulate, int B, int H, int W, int planes, void* stream) {
  SST_REQUIRE(sr && gt && maps && dsr, "sst_ssim_loss_bwd: null pointer");
  if (int rc = ssim_check_shape("sst_ssim_loss_bwd", B, H, W, planes)) return rc;
  dim3 grid((W + LT - 1) / LT, (H + LT - 1) / LT, B * planes);
  const double count = (double)B * planes * (double)(H - LA) * (double)(W - LA);
  ssim_loss_bwd_kernel<<<grid, LNT, 0, sst_stream(stream)>>>(sr, gt, maps, dsr, scale_dev, -(double)scale_host / count, accumulate, H, W,
                                                             planes, ssim_taps());
  SST_LAUNCH_CHECK("ssim_loss_bwd_kernel");
  return SST_OK;
}
