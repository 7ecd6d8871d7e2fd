// Validation metrics on the device (metrics.py: image_metrics_device): per image the MSE of the Y channel on the 0..255 scale over
// all H*W pixels and the mean of the SSIM map over its (H-10) x (W-10) valid region - validate.image_metrics restated rounding for
// rounding, not approximated:
//   q  = rint(clamp(x, 0, 1) * 255.f)                                  fp32, half to even            (utils.tensor2img)
//   v  = fp32(fp32(q / 255.f) * 255.f)                                 fp32                          (image_metrics, bgr2ycbcr's * 255)
//   Y  = fp32(((B*24.966 + G*128.553 + R*65.481) / 255 + 16) / 255)    fp64, rounded to fp32 once    (bgr2ycbcr .. astype(float32))
//   y  = fp32(Y * 255.f)                                               fp32 - what PSNR and SSIM get
// and everything after that in fp64: squared differences, the 11-tap sigma 1.5 Gaussian (normalised in fp64 as
// utils._gaussian_window does, applied separably to x, y, x^2, y^2, xy), the SSIM quotient, all sums.  fp32 is no option for
// sigma^2 = E[x^2] - mu^2 on the 0..255 scale (cancellation error about 65025 * 2^-24 = 4e-3 against C2 = 58.5).
//
// The library is built with -ffp-contract=fast; this file turns contraction OFF, so that every product and sum below rounds where
// the host's does, and spells fma() out where fusing is wanted (the filter taps: summation-order noise only).
//
// One workgroup per 32 x 32 tile and image.  The tile OWNS input pixels [y0, y0+32) x [x0, x0+32) (squared difference, uint8
// output) and the SSIM outputs of the same index range; output (oy, ox) reads inputs [oy, oy+10] x [ox, ox+10], so the workgroup
// stages the tile plus a 10-px apron to the right and below - each pixel quantised and converted once per tile that touches it -
// as two fp32 Y planes in LDS.  Two half tiles of 16 output rows each: horizontal pass of the five quantities into LDS (26 rows),
// vertical pass + SSIM quotient per owned, valid output.  Wave shuffle reduction, ONE fp64 partial pair per workgroup into the
// workspace; sst_image_metrics's second launch sums each image's partials in index order: no floating-point atomics, bit-identical
// from run to run.
//
// NaN: the clamp is written with comparisons that keep NaN (fminf / fmaxf would drop it), so a NaN anywhere in sr or hr makes that
// image's MSE and SSIM NaN (every pixel lies in at least one SSIM window).  The uint8 output of a NaN pixel is 0.
#include "common.h"
#include "pixel_io.h"      // quantise, to_u8: tensor2img's quantisation

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int MT = 32;                 // tile edge (owned pixels / outputs)
constexpr int MK = 11;                 // Gaussian taps
constexpr int MS = MT + MK - 1;        // staged edge: 42
constexpr int MSP = MS + 1;            // LDS row pitch of the staged planes
constexpr int MHALF = 16;              // output rows per half tile
constexpr int MHR = MHALF + MK - 1;    // horizontal-pass rows per half tile: 26
constexpr int MNT = 256;
constexpr int FIN_NT = 256;

constexpr double SSIM_C1 = (0.01 * 255) * (0.01 * 255);
constexpr double SSIM_C2 = (0.03 * 255) * (0.03 * 255);

struct MetricTaps {
  double w[MK];
};

// utils._gaussian_window's 1-D factor: exp(-(x*x) / (2*sigma*sigma)) / sum, the sum taken the way numpy's pairwise add takes 11 terms
static MetricTaps metric_taps() {
  MetricTaps t;
  const double sigma = 1.5;
  for (int i = 0; i < MK; ++i) {
    const double x = (double)i - (MK - 1) / 2.0;
    t.w[i] = std::exp(-(x * x) / (2.0 * sigma * sigma));
  }
  double s = ((t.w[0] + t.w[1]) + (t.w[2] + t.w[3])) + ((t.w[4] + t.w[5]) + (t.w[6] + t.w[7]));
  for (int i = 8; i < MK; ++i) s += t.w[i];
  for (int i = 0; i < MK; ++i) t.w[i] /= s;
  return t;
}

// the value PSNR / SSIM receive for one pixel from its three quantised channels (0..255, RGB order)
__device__ __forceinline__ float luma255(float qr, float qg, float qb) {
  const float vr = (qr / 255.f) * 255.f, vg = (qg / 255.f) * 255.f, vb = (qb / 255.f) * 255.f;
  double y = ((double)vb * 24.966 + (double)vg * 128.553) + (double)vr * 65.481;
  y = y / 255.0 + 16.0;
  y = y / 255.0;
  return (float)y * 255.f;
}

__global__ __launch_bounds__(MNT) void image_metrics_kernel(const float* __restrict__ sr, const float* __restrict__ hr, int H, int W,
                                                            uint8_t* __restrict__ sr_u8, uint8_t* __restrict__ hr_u8,
                                                            double* __restrict__ partials, MetricTaps taps) {
  __shared__ float s_x[MS * MSP], s_y[MS * MSP];
  __shared__ double s_h[5][MHR][MT];
  __shared__ double s_red[2][MNT / 64];
  const int tid = threadIdx.x, b = blockIdx.z;
  const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
  const int64_t plane = (int64_t)H * W;
  const float* srb = sr + (int64_t)b * 3 * plane;
  const float* hrb = hr + (int64_t)b * 3 * plane;

  // ---- stage: quantise + Y, once per staged pixel; owned pixels also give the squared difference and the uint8 images
  double se = 0.0;
  for (int i = tid; i < MS * MS; i += MNT) {
    const int r = i / MS, c = i - r * MS;
    const int gy = y0 + r, gx = x0 + c;
    float xs = 0.f, ys = 0.f;
    if (gy < H && gx < W) {
      const int64_t o = (int64_t)gy * W + gx;
      const float sq0 = quantise(srb[o]), sq1 = quantise(srb[o + plane]), sq2 = quantise(srb[o + 2 * plane]);
      const float hq0 = quantise(hrb[o]), hq1 = quantise(hrb[o + plane]), hq2 = quantise(hrb[o + 2 * plane]);
      xs = luma255(sq0, sq1, sq2);
      ys = luma255(hq0, hq1, hq2);
      if (r < MT && c < MT) {
        const double d = (double)xs - (double)ys;
        se += d * d;
        const int64_t u = ((int64_t)b * plane + o) * 3;
        if (sr_u8) {
          sr_u8[u] = to_u8(sq2);
          sr_u8[u + 1] = to_u8(sq1);
          sr_u8[u + 2] = to_u8(sq0);
        }
        if (hr_u8) {
          hr_u8[u] = to_u8(hq2);
          hr_u8[u + 1] = to_u8(hq1);
          hr_u8[u + 2] = to_u8(hq0);
        }
      }
    }
    s_x[r * MSP + c] = xs;
    s_y[r * MSP + c] = ys;
  }
  __syncthreads();

  double ss = 0.0;
  for (int half = 0; half < MT / MHALF; ++half) {
    // ---- horizontal pass: rows [16*half, 16*half + 26) of the staged planes, 32 columns, five quantities
    for (int i = tid; i < MHR * MT; i += MNT) {
      const int rr = i / MT, c = i % MT;
      const float* px = s_x + (half * MHALF + rr) * MSP + c;
      const float* py = s_y + (half * MHALF + rr) * MSP + c;
      double ax = 0.0, ay = 0.0, axx = 0.0, ayy = 0.0, axy = 0.0;
#pragma unroll
      for (int t = 0; t < MK; ++t) {
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
    // ---- vertical pass + SSIM quotient: 16 x 32 outputs, two per thread
    for (int i = tid; i < MHALF * MT; i += MNT) {
      const int j = i / MT, c = i % MT;
      const int oy = y0 + half * MHALF + j, ox = x0 + c;
      if (oy <= H - MK && ox <= W - MK) {
        double mu1 = 0.0, mu2 = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
        for (int t = 0; t < MK; ++t) {
          const double w = taps.w[t];
          mu1 = fma(w, s_h[0][j + t][c], mu1);
          mu2 = fma(w, s_h[1][j + t][c], mu2);
          exx = fma(w, s_h[2][j + t][c], exx);
          eyy = fma(w, s_h[3][j + t][c], eyy);
          exy = fma(w, s_h[4][j + t][c], exy);
        }
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const double sigma1_sq = exx - mu1_sq, sigma2_sq = eyy - mu2_sq, sigma12 = exy - mu1_mu2;
        ss += ((2.0 * mu1_mu2 + SSIM_C1) * (2.0 * sigma12 + SSIM_C2)) /
              ((mu1_sq + mu2_sq + SSIM_C1) * (sigma1_sq + sigma2_sq + SSIM_C2));
      }
    }
    __syncthreads();
  }

  // ---- one partial pair per workgroup
  se = wave_sum_d(se);
  ss = wave_sum_d(ss);
  if ((tid & 63) == 0) {
    s_red[0][tid >> 6] = se;
    s_red[1][tid >> 6] = ss;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, c = 0.0;
#pragma unroll
    for (int k = 0; k < MNT / 64; ++k) {
      a += s_red[0][k];
      c += s_red[1][k];
    }
    const int64_t tile = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * tile] = a;
    partials[2 * tile + 1] = c;
  }
}

// one workgroup per image: its tiles' partials in index order
__global__ __launch_bounds__(FIN_NT) void image_metrics_finalize_kernel(const double* __restrict__ partials, int ntile, int H, int W,
                                                                        double* __restrict__ out) {
  __shared__ double red[FIN_NT / 64];
  const int b = blockIdx.x;
  const double* p = partials + (int64_t)b * ntile * 2;
  double a = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < ntile; i += FIN_NT) {
    a += p[2 * i];
    c += p[2 * i + 1];
  }
  a = block_sum_d<FIN_NT>(a, red);
  c = block_sum_d<FIN_NT>(c, red);
  if (threadIdx.x == 0) {
    out[2 * b] = a / ((double)H * (double)W);
    out[2 * b + 1] = c / ((double)(H - MK + 1) * (double)(W - MK + 1));
  }
}

}  // namespace

SST_API int sst_image_metrics_workspace(int B, int H, int W, int64_t* partial_doubles) {
  SST_REQUIRE(B > 0 && H > 0 && W > 0 && partial_doubles, "sst_image_metrics_workspace: bad shape");
  *partial_doubles = 2 * (int64_t)B * ((H + MT - 1) / MT) * ((W + MT - 1) / MT);
  return SST_OK;
}

SST_API int sst_image_metrics(const float* sr, const float* hr, int B, int H, int W, double* out, uint8_t* sr_u8, uint8_t* hr_u8,
                              double* workspace, void* stream) {
  SST_REQUIRE(sr && hr && out && workspace, "sst_image_metrics: null pointer");
  SST_REQUIRE(B > 0 && B <= 65535, "sst_image_metrics: bad batch %d", B);
  SST_REQUIRE(H >= MK && W >= MK, "sst_image_metrics: image %dx%d is below the 11-px minimum of the SSIM window", W, H);
  const int ntx = (W + MT - 1) / MT, nty = (H + MT - 1) / MT;
  SST_REQUIRE(nty <= 65535, "sst_image_metrics: image height %d needs more than 65535 tile rows", H);
  image_metrics_kernel<<<dim3(ntx, nty, B), MNT, 0, sst_stream(stream)>>>(sr, hr, H, W, sr_u8, hr_u8, workspace, metric_taps());
  SST_LAUNCH_CHECK("image_metrics_kernel");
  image_metrics_finalize_kernel<<<B, FIN_NT, 0, sst_stream(stream)>>>(workspace, ntx * nty, H, W, out);
  SST_LAUNCH_CHECK("image_metrics_finalize_kernel");
  return SST_OK;
}
