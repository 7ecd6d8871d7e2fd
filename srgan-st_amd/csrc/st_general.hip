// Structure-tensor loss and maps at any (sigma, rho) with radii R1 <= 8, R2 <= 20, for gfx950: the separable path next to the two
// 32x32-tile builds of st_loss.hip / st_maps.hip.
//
// Replaces (reference file:line)
//   StructureTensorLoss.forward / st_loss          loss.py:399-413   for every sigma / rho the tile kernels do not instantiate
//   structure_tensor                                utils.py:212-233  (10 separable 'same' zero-padded correlations)
//   get_gaussian_kernel                             utils.py:194-208  (taps computed on the host, passed by value)
//
// The tile kernels stage a (32 + 2 (R1 + R2))^2 patch per tile, which at radii (8, 20) is 88 x 88 px for 32 x 32 outputs and more LDS
// than a workgroup has.  Here every one of the ten correlations is a 1-D pass over whole planes kept in a caller-provided
// workspace; a workgroup of 256 threads produces a 32 x 32 tile of one pass from a strip of 32 x (32 + 2 R) values staged in LDS
// (zero outside the image, which IS the reference's zero padding of every intermediate).  Radii are runtime values: one build.
//
//   forward   a  gray -> H pass (dg, g)   -> A1, A2        [2B planes: sr then gt]
//             b  W pass (g, dg)           -> Ix, Iy        (Ix, Iy of sr are the caller's `saved` planes: the backward reads them)
//             c  products, H pass (k)     -> Q  [2B,3]
//             d  W pass (k) of both images, pointwise chain, gS, block sums, last-block ticket -> gS [B,3,H,W], loss
//   backward  e  H pass (k) on gS         -> U  [B,3]
//             f  W pass (k), dIx = 2 Ix gJxx + Iy gJxy, dIy = 2 Iy gJyy + Ix gJxy   (Ix, Iy saved by the forward)
//             g  W adjoint (g, -dg)       -> dA1, dA2
//             h  H adjoint (-dg, g), gray weights, scale, (accumulate) -> dsr
//   maps      a b c, then the W pass (k) -> S [2B,3], then a pointwise kernel -> Sx, Sgt, Fx, Fgt, d, tile sums (st_maps.hip's layout)
//
// Taps live in the kernel argument block and are only ever indexed by unrolled, compile-time indices (uniform loads into SGPRs):
// nothing is indexed at run time in private memory, so no kernel here uses scratch.
#include "st_tile.h"

namespace {

constexpr int GNT = 256;                 // threads per workgroup
constexpr int GPP = T * T / GNT;       // outputs per thread
constexpr int MAXR1 = 8, MAXR2 = 20;     // the bound of this path
constexpr int S1 = T * (T + 2 * MAXR1);   // floats of one staged strip, derivative / integration radius
constexpr int S2 = T * (T + 2 * MAXR2);

struct StgTaps {
  float g[2 * MAXR1 + 1];
  float dg[2 * MAXR1 + 1];
  float k[2 * MAXR2 + 1];
};

// Image n of a two-part batch: planes of the first nb images at a, of the rest at b (each image `per` floats).
struct Split {
  float* a;
  float* b;
  int nb;
};
__device__ __forceinline__ float* part(const Split& s, int n, size_t per) {
  return n < s.nb ? s.a + (size_t)n * per : s.b + (size_t)(n - s.nb) * per;
}

// Strip for a pass along H: s[T + 2r][T] = plane rows y0 - r .., columns x0 ..; zero outside the image.
__device__ __forceinline__ void stage_cols(const float* __restrict__ p, int H, int W, int y0, int x0, int r, float* s) {
  const int n = (T + 2 * r) * T;
  for (int i = threadIdx.x; i < n; i += GNT) {
    const int y = y0 - r + (i >> 5), x = x0 + (i & 31);
    s[i] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? p[(size_t)y * W + x] : 0.f;
  }
}
// Strip for a pass along W: s[T][T + 2r] = plane rows y0 .., columns x0 - r ..; zero outside the image.
__device__ __forceinline__ void stage_rows(const float* __restrict__ p, int H, int W, int y0, int x0, int r, float* s) {
  const int rs = T + 2 * r, n = T * rs;
  for (int i = threadIdx.x; i < n; i += GNT) {
    const int pr = i / rs, pc = i - pr * rs;
    const int y = y0 + pr, x = x0 - r + pc;
    s[i] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? p[(size_t)y * W + x] : 0.f;
  }
}

// for (t = 0 .. 2r) with t a compile-time constant in the body: the taps stay in SGPRs
#define STG_TAPS(MAXR, r, t) \
  _Pragma("unroll") for (int t = 0; t <= 2 * (MAXR); ++t) \
    if (t <= 2 * (r))

// ---------------------------------------------------------------------------------------------- a
// gray, then A1 = dg (x)_H gray, A2 = g (x)_H gray                                              utils.py:219,221
__global__ __launch_bounds__(GNT) void stg_gray_hpass_kernel(const float* __restrict__ x, const float* __restrict__ gt, int B,
                                                             float* __restrict__ A1, float* __restrict__ A2, int H, int W, int r1,
                                                             StgTaps tp) {
  __shared__ float s[S1];
  const int n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W;
  const float* img = n < B ? x + (size_t)n * 3 * hw : gt + (size_t)(n - B) * 3 * hw;
  const int ns = (T + 2 * r1) * T;
  for (int i = threadIdx.x; i < ns; i += GNT) s[i] = gray_at(img, H, W, y0 - r1 + (i >> 5), x0 + (i & 31));
  __syncthreads();
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float a1 = 0.f, a2 = 0.f;
    STG_TAPS(MAXR1, r1, t) {
      const float v = s[(row + t) * T + col];
      a1 = fmaf(tp.dg[t], v, a1);
      a2 = fmaf(tp.g[t], v, a2);
    }
    const int y = y0 + row, xx = x0 + col;
    if (y < H && xx < W) {
      const size_t o = (size_t)n * hw + (size_t)y * W + xx;
      A1[o] = a1;
      A2[o] = a2;
    }
  }
}

// ---------------------------------------------------------------------------------------------- b
// Ix = g (x)_W A1, Iy = dg (x)_W A2                                                             utils.py:220,222
__global__ __launch_bounds__(GNT) void stg_wpass_grad_kernel(const float* __restrict__ A1, const float* __restrict__ A2, Split Ix,
                                                             Split Iy, int H, int W, int r1, StgTaps tp) {
  __shared__ float s1[S1], s2[S1];
  const int n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T, rs = T + 2 * r1;
  const size_t hw = (size_t)H * W;
  stage_rows(A1 + (size_t)n * hw, H, W, y0, x0, r1, s1);
  stage_rows(A2 + (size_t)n * hw, H, W, y0, x0, r1, s2);
  __syncthreads();
  float* ox = part(Ix, n, hw);
  float* oy = part(Iy, n, hw);
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float ix = 0.f, iy = 0.f;
    STG_TAPS(MAXR1, r1, t) {
      ix = fmaf(tp.g[t], s1[row * rs + col + t], ix);
      iy = fmaf(tp.dg[t], s2[row * rs + col + t], iy);
    }
    const int y = y0 + row, xx = x0 + col;
    if (y < H && xx < W) {
      ox[(size_t)y * W + xx] = ix;
      oy[(size_t)y * W + xx] = iy;
    }
  }
}

// ---------------------------------------------------------------------------------------------- c
// Q = k (x)_H (Ix^2, Iy^2, Ix Iy), the products formed on load                                  utils.py:225,227,229
__global__ __launch_bounds__(GNT) void stg_hpass_products_kernel(Split Ix, Split Iy, float* __restrict__ Q, int H, int W, int r2,
                                                                 StgTaps tp) {
  __shared__ float s1[S2], s2[S2];
  const int n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W;
  stage_cols(part(Ix, n, hw), H, W, y0, x0, r2, s1);
  stage_cols(part(Iy, n, hw), H, W, y0, x0, r2, s2);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
    STG_TAPS(MAXR2, r2, t) {
      const float ix = s1[(row + t) * T + col], iy = s2[(row + t) * T + col];
      q0 = fmaf(tp.k[t], ix * ix, q0);
      q1 = fmaf(tp.k[t], iy * iy, q1);
      q2 = fmaf(tp.k[t], ix * iy, q2);
    }
    const int y = y0 + row, xx = x0 + col;
    if (y < H && xx < W) {
      const size_t o = (size_t)n * 3 * hw + (size_t)y * W + xx;
      store_planes(Q, o, hw, q0, q1, q2);
    }
  }
}

// k (x)_W on the three planes of one image at src ([3][H][W]) -> J of this thread's GPP pixels.  s: 3 * S2 floats.   utils.py:226,228,230
__device__ __forceinline__ void wpass_three(const float* __restrict__ src, int H, int W, int y0, int x0, int r2, const StgTaps& tp,
                                            float* s, float (&J)[GPP][3]) {
  const size_t hw = (size_t)H * W;
  const int rs = T + 2 * r2;
  __syncthreads();  // previous user of the LDS is done
#pragma unroll
  for (int c = 0; c < 3; ++c) stage_rows(src + c * hw, H, W, y0, x0, r2, s + c * S2);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    STG_TAPS(MAXR2, r2, t) {
      const float kk = tp.k[t];
      v0 = fmaf(kk, s[row * rs + col + t], v0);
      v1 = fmaf(kk, s[S2 + row * rs + col + t], v1);
      v2 = fmaf(kk, s[2 * S2 + row * rs + col + t], v2);
    }
    J[j][0] = v0;
    J[j][1] = v1;
    J[j][2] = v2;
  }
}

// ---------------------------------------------------------------------------------------------- d
// Q: [2B][3][H][W], image b of sr at b, of gt at B + b.  The gradient of d is st_loss_fwd_kernel's (st_tile.h) with its eigenvalue
// half on a discriminant that does not cancel (below).
__global__ __launch_bounds__(GNT) void stg_loss_fwd_kernel(const float* __restrict__ Q, float* __restrict__ gS, float* __restrict__ loss,
                                                           float* __restrict__ partials, unsigned* __restrict__ counter, int B, int H,
                                                           int W, int r2, int normalize, StgTaps tp) {
  __shared__ float s[3 * S2];
  __shared__ float red[GNT / 64];
  __shared__ unsigned s_flag;
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W, img_off = (size_t)b * 3 * hw;
  float J1[GPP][3], J2[GPP][3];
  wpass_three(Q + img_off, H, W, y0, x0, r2, tp, s, J1);
  wpass_three(Q + (size_t)(B + b) * 3 * hw, H, W, y0, x0, r2, tp, s, J2);

  const float eps = 1e-12f;
  float lsum = 0.f;
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, y = y0 + (p >> 5), x = x0 + (p & 31);
    if (y >= H || x >= W) continue;
    const float a1 = J1[j][0], b1 = J1[j][1], c1 = J1[j][2];
    const StPoint pt = st_pointwise(a1, b1, c1, J2[j][0], J2[j][1], J2[j][2], normalize);
    lsum += pt.d;

    // ---- analytic gradient of d wrt (a1,b1,c1), unit upstream.  The tile kernel differentiates the forward's own values; here the
    // eigenvalue half is re-evaluated from disc = (A - Bm)^2 + 4 C D, the same discriminant as ApB^2 - 4 (A Bm - C D) without
    // its cancellation.  Wide kernels smooth sr and gt towards each other, both eigenvalues approach 1, ApB^2 and 4 det agree to
    // ~1e-7 and their fp32 difference keeps few or no correct digits: harmless for d (the loss keeps pt.d), but d has a square
    // root's singularity at disc = 0, its derivative goes with 1 / r, and the clamp's gate flips on that noise.
    const float AmB = pt.A - pt.Bm;
    const float disc = AmB * AmB + 4.f * pt.C * pt.D;
    const float r = sqrtf(disc < eps ? eps : disc);
    const float l1 = 0.5f * (pt.ApB - r), l2 = 0.5f * (pt.ApB + r);
    const float L1 = l1 < 1.f ? 1.f : l1, L2 = l2 < 1.f ? 1.f : l2;     // NaN stays NaN, as in st_pointwise
    const float g1 = logf(L1), g2 = logf(L2);
    const float d = sqrtf(g1 * g1 + g2 * g2 + eps);
    const StEigGrad e = st_grad_eigen(d, l1, l2, L1, L2, g1, g2, disc, r);
    const float dApB = 0.5f * e.dl12;
    const float dA = dApB + e.ddisc * 2.f * AmB;        // = dApB + ddisc * (2 ApB - 4 Bm), the tile kernel's form
    const float dB = dApB - e.ddisc * 2.f * AmB;
    const float dC = 4.f * e.ddisc * pt.D;
    const float dD = 4.f * e.ddisc * pt.C;
    st_grad_store(gS, img_off + (size_t)y * W + x, hw, dA, dB, dC, dD, pt, a1, b1, c1, normalize);
  }
  const float bsum = block_sum<GNT>(lsum, red);
  const unsigned nblk = gridDim.x * gridDim.y * gridDim.z;
  const unsigned me = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (threadIdx.x == 0) partials[me] = bsum;
  float tot;
  if (last_block_total<GNT>(partials, counter, nblk, &s_flag, red, tot)) {   // re-arms the counter: graph replays work
    if (threadIdx.x == 0) loss[0] = tot / ((float)B * (float)H * (float)W);
  }
}

// ---------------------------------------------------------------------------------------------- maps
// S = k (x)_W Q for every image: [nimg][3][H][W]
__global__ __launch_bounds__(GNT) void stg_wpass_tensor_kernel(const float* __restrict__ Q, float* __restrict__ S, int H, int W, int r2,
                                                               StgTaps tp) {
  __shared__ float s[3 * S2];
  const int n = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W, img_off = (size_t)n * 3 * hw;
  float J[GPP][3];
  wpass_three(Q + img_off, H, W, y0, x0, r2, tp, s, J);
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, y = y0 + (p >> 5), x = x0 + (p & 31);
    if (y >= H || x >= W) continue;
    const size_t o = img_off + (size_t)y * W + x;
    store_planes(S, o, hw, J[j][0], J[j][1], J[j][2]);
  }
}

// S: [B (+ B)][3][H][W] (gt's images behind x's; absent when has_gt is 0) -> the outputs of sst_st_maps, same layouts
__global__ __launch_bounds__(GNT) void stg_maps_point_kernel(const float* __restrict__ S, StMapsOut out, int B, int H, int W,
                                                             int has_gt, int normalize) {
  __shared__ float red[GNT / 64];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W;
  float lsum = 0.f;
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, y = y0 + (p >> 5), xx = x0 + (p & 31);
    if (y >= H || xx >= W) continue;                    // outside the image: neither stored nor summed
    const size_t px = (size_t)y * W + xx, o = (size_t)b * 3 * hw + px;
    const float J1[3] = {S[o], S[o + hw], S[o + 2 * hw]};
    float J2[3] = {0.f, 0.f, 0.f};
    if (has_gt) {
      const size_t o2 = (size_t)(B + b) * 3 * hw + px;
      J2[0] = S[o2], J2[1] = S[o2 + hw], J2[2] = S[o2 + 2 * hw];
    }
    maps_pixel(out, b, px, hw, J1, J2, normalize, lsum);
  }
  maps_tile_sum<GNT>(out, b, lsum, red);
}

// ---------------------------------------------------------------------------------------------- e
// adjoint of the integration passes (k symmetric), along H: U = k (x)_H gS, three planes per image
__global__ __launch_bounds__(GNT) void stg_hpass_three_kernel(const float* __restrict__ gS, float* __restrict__ U, int H, int W, int r2,
                                                              StgTaps tp) {
  __shared__ float s[3 * S2];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W, img_off = (size_t)b * 3 * hw;
#pragma unroll
  for (int c = 0; c < 3; ++c) stage_cols(gS + img_off + c * hw, H, W, y0, x0, r2, s + c * S2);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float u0 = 0.f, u1 = 0.f, u2 = 0.f;
    STG_TAPS(MAXR2, r2, t) {
      const float kk = tp.k[t];
      u0 = fmaf(kk, s[(row + t) * T + col], u0);
      u1 = fmaf(kk, s[S2 + (row + t) * T + col], u1);
      u2 = fmaf(kk, s[2 * S2 + (row + t) * T + col], u2);
    }
    const int y = y0 + row, xx = x0 + col;
    if (y < H && xx < W) {
      const size_t o = img_off + (size_t)y * W + xx;
      store_planes(U, o, hw, u0, u1, u2);
    }
  }
}

// ---------------------------------------------------------------------------------------------- f
// ... along W, then dIx = 2 Ix gJxx + Iy gJxy, dIy = 2 Iy gJyy + Ix gJxy with the forward's Ix, Iy of sr (saved: [2][B][H][W])
__global__ __launch_bounds__(GNT) void stg_wpass_dgrad_kernel(const float* __restrict__ U, const float* __restrict__ saved,
                                                              float* __restrict__ dIx, float* __restrict__ dIy, int B, int H, int W,
                                                              int r2, StgTaps tp) {
  __shared__ float s[3 * S2];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W;
  float V[GPP][3];
  wpass_three(U + (size_t)b * 3 * hw, H, W, y0, x0, r2, tp, s, V);
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, y = y0 + (p >> 5), x = x0 + (p & 31);
    if (y >= H || x >= W) continue;
    const size_t o = (size_t)b * hw + (size_t)y * W + x;
    const float ix = saved[o], iy = saved[(size_t)B * hw + o];
    dIx[o] = 2.f * ix * V[j][0] + iy * V[j][2];
    dIy[o] = 2.f * iy * V[j][1] + ix * V[j][2];
  }
}

// ---------------------------------------------------------------------------------------------- g
// adjoint of the W passes: dA1 = g (x)_W dIx ; dA2 = flip(dg) (x)_W dIy = -(dg (x)_W dIy)
__global__ __launch_bounds__(GNT) void stg_wadj_kernel(const float* __restrict__ dIx, const float* __restrict__ dIy,
                                                       float* __restrict__ dA1, float* __restrict__ dA2, int H, int W, int r1,
                                                       StgTaps tp) {
  __shared__ float s1[S1], s2[S1];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T, rs = T + 2 * r1;
  const size_t hw = (size_t)H * W;
  stage_rows(dIx + (size_t)b * hw, H, W, y0, x0, r1, s1);
  stage_rows(dIy + (size_t)b * hw, H, W, y0, x0, r1, s2);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float d1 = 0.f, d2 = 0.f;
    STG_TAPS(MAXR1, r1, t) {
      d1 = fmaf(tp.g[t], s1[row * rs + col + t], d1);
      d2 = fmaf(-tp.dg[t], s2[row * rs + col + t], d2);
    }
    const int y = y0 + row, xx = x0 + col;
    if (y < H && xx < W) {
      const size_t o = (size_t)b * hw + (size_t)y * W + xx;
      dA1[o] = d1;
      dA2[o] = d2;
    }
  }
}

// ---------------------------------------------------------------------------------------------- h
// adjoint of the H passes: dG = flip(dg) (x)_H dA1 + g (x)_H dA2; d(sr) (+)= gray_w[c] * scale * dG,
// scale = scale_host * (scale_dev ? *scale_dev : 1)
__global__ __launch_bounds__(GNT) void stg_hadj_out_kernel(const float* __restrict__ dA1, const float* __restrict__ dA2,
                                                           float* __restrict__ dsr, const float* __restrict__ scale_dev,
                                                           float scale_host, int accumulate, int H, int W, int r1, StgTaps tp) {
  __shared__ float s1[S1], s2[S1];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W;
  stage_cols(dA1 + (size_t)b * hw, H, W, y0, x0, r1, s1);
  stage_cols(dA2 + (size_t)b * hw, H, W, y0, x0, r1, s2);
  __syncthreads();
  float scale = scale_host;
  if (scale_dev) scale *= scale_dev[0];
#pragma unroll
  for (int j = 0; j < GPP; ++j) {
    const int p = threadIdx.x + j * GNT, row = p >> 5, col = p & 31;
    float dg_ = 0.f;
    STG_TAPS(MAXR1, r1, t) {
      dg_ = fmaf(-tp.dg[t], s1[(row + t) * T + col], dg_);
      dg_ = fmaf(tp.g[t], s2[(row + t) * T + col], dg_);
    }
    const int y = y0 + row, xx = x0 + col;
    if (y < H && xx < W) {
      const size_t o = (size_t)b * 3 * hw + (size_t)y * W + xx;
      store_gray_grad(dsr, o, hw, dg_ * scale, accumulate, nullptr);
    }
  }
}

// ---------------------------------------------------------------------------------------------- host
StgTaps make_taps_rt(float sigma, float rho, int r1, int r2) {
  StgTaps tp = {};
  gaussian_taps(sigma, r1, tp.g, tp.dg);
  gaussian_taps(rho, r2, tp.k, nullptr);
  return tp;
}

// 0: a tile build (st_loss.hip / st_maps.hip), 1: this file, SST_ERR_UNSUPPORTED beyond the bound
int st_route(const char* who, float sigma, float rho, int* r1, int* r2) {
  if (!(fabsf(sigma) < 1e6f && fabsf(rho) < 1e6f)) return sst_set_error(SST_ERR_ARG, "%s: sigma / rho must be finite", who);
  *r1 = radius_of(sigma), *r2 = radius_of(rho);
  if (with_tile_build(*r1, *r2, [](auto, auto) {})) return 0;
  if (*r1 <= MAXR1 && *r2 <= MAXR2) return 1;
  return sst_set_error(SST_ERR_UNSUPPORTED, "%s: (sigma,rho)=(%g,%g) -> radii (%d,%d) not built", who, sigma, rho, *r1, *r2);
}

// B up to 32767: the grid's z carries 2 B images; the 14 B H W floats of the scratch are kept to 2^40 elements
bool general_shape_ok(int B, int H, int W) { return shape_ok(B, H, W, 32767) && (int64_t)B * H * W <= (int64_t)1 << 40; }

// passes a, b, c for nimg images (x's B, then gt's when gt != null): Q at `Q`
void launch_abc(const float* x, const float* gt, int B, int nimg, float* A1, float* A2, Split Ix, Split Iy, float* Q, int H, int W, int r1,
                int r2, const StgTaps& tp, hipStream_t st) {
  const dim3 grid = tiles_grid(H, W, nimg);
  stg_gray_hpass_kernel<<<grid, GNT, 0, st>>>(x, gt, B, A1, A2, H, W, r1, tp);
  stg_wpass_grad_kernel<<<grid, GNT, 0, st>>>(A1, A2, Ix, Iy, H, W, r1, tp);
  stg_hpass_products_kernel<<<grid, GNT, 0, st>>>(Ix, Iy, Q, H, W, r2, tp);
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
// Host only.  0: (sigma, rho) selects a tile build, 1: the general path, SST_ERR_UNSUPPORTED: R1 > 8 or R2 > 20.
SST_API int sst_st_route(float sigma, float rho, int* r1, int* r2) {
  SST_REQUIRE(r1 && r2, "sst_st_route: null pointer");
  return st_route("sst_st_route", sigma, rho, r1, r2);
}

// Floats of the general path's buffers with N = B*H*W: scratch 14 N (forward 12 N, backward 7 N, maps 14 N: one buffer serves all),
// saved 2 N (Ix, Iy of sr: written by the forward, read by the backward), partials B * ceil(H/32) * ceil(W/32).
SST_API int sst_st_general_workspace(int B, int H, int W, int64_t* scratch_floats, int64_t* saved_floats, int64_t* partial_floats) {
  SST_REQUIRE(general_shape_ok(B, H, W) && scratch_floats && saved_floats && partial_floats, "sst_st_general_workspace: bad shape");
  const int64_t n = (int64_t)B * H * W;
  *scratch_floats = 14 * n;
  *saved_floats = 2 * n;
  *partial_floats = tiles_of(B, H, W);
  return SST_OK;
}

SST_API int sst_st_general_fwd(const float* sr, const float* gt, float* loss, float* gS, float* saved, float* scratch, float* partials,
                               unsigned* counter, int B, int H, int W, float sigma, float rho, int normalize, void* stream) {
  SST_REQUIRE(sr && gt && loss && gS && saved && scratch && partials && counter, "sst_st_general_fwd: null pointer");
  SST_REQUIRE(general_shape_ok(B, H, W), "sst_st_general_fwd: bad shape B=%d H=%d W=%d", B, H, W);
  int r1, r2;
  const int route = st_route("sst_st_general_fwd", sigma, rho, &r1, &r2);
  if (route < 0) return route;
  const size_t n = (size_t)B * H * W;
  const StgTaps tp = make_taps_rt(sigma, rho, r1, r2);
  hipStream_t st = sst_stream(stream);
  float *A1 = scratch, *A2 = scratch + 2 * n, *Igt = scratch + 4 * n, *Q = scratch + 6 * n;     // 2n 2n 2n 6n
  launch_abc(sr, gt, B, 2 * B, A1, A2, Split{saved, Igt, B}, Split{saved + n, Igt + n, B}, Q, H, W, r1, r2, tp, st);
  stg_loss_fwd_kernel<<<tiles_grid(H, W, B), GNT, 0, st>>>(Q, gS, loss, partials, counter, B, H, W, r2, normalize, tp);
  SST_LAUNCH_CHECK("stg_loss_fwd_kernel");
  return SST_OK;
}

// dsr (+)= scale_host * (scale_dev ? *scale_dev : 1) * d loss / d sr, from the forward's gS and saved planes
SST_API int sst_st_general_bwd(const float* saved, const float* gS, float* dsr, float* scratch, const float* scale_dev, float scale_host,
                               int accumulate, int B, int H, int W, float sigma, float rho, void* stream) {
  SST_REQUIRE(saved && gS && dsr && scratch, "sst_st_general_bwd: null pointer");
  SST_REQUIRE(general_shape_ok(B, H, W), "sst_st_general_bwd: bad shape B=%d H=%d W=%d", B, H, W);
  int r1, r2;
  const int route = st_route("sst_st_general_bwd", sigma, rho, &r1, &r2);
  if (route < 0) return route;
  const size_t n = (size_t)B * H * W;
  const StgTaps tp = make_taps_rt(sigma, rho, r1, r2);
  hipStream_t st = sst_stream(stream);
  float *U = scratch, *dIx = scratch + 3 * n, *dIy = scratch + 4 * n, *dA1 = scratch + 5 * n, *dA2 = scratch + 6 * n;
  const dim3 grid = tiles_grid(H, W, B);
  const float s = scale_host / ((float)B * (float)H * (float)W);
  stg_hpass_three_kernel<<<grid, GNT, 0, st>>>(gS, U, H, W, r2, tp);
  stg_wpass_dgrad_kernel<<<grid, GNT, 0, st>>>(U, saved, dIx, dIy, B, H, W, r2, tp);
  stg_wadj_kernel<<<grid, GNT, 0, st>>>(dIx, dIy, dA1, dA2, H, W, r1, tp);
  stg_hadj_out_kernel<<<grid, GNT, 0, st>>>(dA1, dA2, dsr, scale_dev, s, accumulate, H, W, r1, tp);
  SST_LAUNCH_CHECK("stg_hadj_out_kernel");
  return SST_OK;
}

// sst_st_maps for every (sigma, rho) within the bound: same outputs, same layouts, plus the scratch buffer
SST_API int sst_st_general_maps(const float* x, const float* gt, float* Sx, float* Sgt, float* Fx, float* Fgt, float* d, float* tile_sums,
                                float* scratch, int B, int H, int W, float sigma, float rho, int normalize, void* stream) {
  SST_REQUIRE(x && scratch, "sst_st_general_maps: null pointer (x / scratch)");
  const StMapsOut out{Sx, Sgt, Fx, Fgt, d, tile_sums};
  if (const int rc = maps_args_ok("sst_st_general_maps", general_shape_ok(B, H, W), B, H, W, gt, out)) return rc;
  int r1, r2;
  const int route = st_route("sst_st_general_maps", sigma, rho, &r1, &r2);
  if (route < 0) return route;
  const size_t n = (size_t)B * H * W;
  const int nimg = gt ? 2 * B : B;
  const StgTaps tp = make_taps_rt(sigma, rho, r1, r2);
  hipStream_t st = sst_stream(stream);
  float *A1 = scratch, *A2 = scratch + 2 * n, *Ix = scratch + 4 * n, *Iy = scratch + 6 * n, *Q = scratch + 8 * n;   // 2n 2n 2n 2n 6n
  float* S = scratch;                                                                                             // over A / I: dead by then
  launch_abc(x, gt, B, nimg, A1, A2, Split{Ix, Ix + n, B}, Split{Iy, Iy + n, B}, Q, H, W, r1, r2, tp, st);
  stg_wpass_tensor_kernel<<<tiles_grid(H, W, nimg), GNT, 0, st>>>(Q, S, H, W, r2, tp);
  stg_maps_point_kernel<<<tiles_grid(H, W, B), GNT, 0, st>>>(S, out, B, H, W, gt ? 1 : 0, normalize);
  SST_LAUNCH_CHECK("stg_maps_point_kernel");
  return SST_OK;
}
