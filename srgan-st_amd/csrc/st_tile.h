// Structure tensor of one 32x32 tile and the pointwise distance chain: the code st_loss.hip (the criterion) and st_maps.hip (the
// analysis maps) both run.  Every translation unit that includes this gets its own copy (unnamed namespace).
//
// Replaces (reference file:line)
//   structure_tensor                                utils.py:212-233   (10 separable 'same' zero-padded correlations)
//   get_gaussian_kernel                             utils.py:194-208   (taps computed on the host, passed by value)
//   normalize / compute_invS1xS2 / compute_eigenvalues / compute_distance   utils.py:236-280
//   torchvision Grayscale                           loss.py:400-401    (0.2989 R + 0.587 G + 0.114 B)
//
// Axis convention - the reference's names, not intuition: utils.py:219 reshapes the derivative taps of Ix to (1,1,-1,1), so "x" is
// the HEIGHT axis (dim -2) and "y" the width axis.  Plane 0 (Jxx) carries the energy of an image that varies only from row to row,
// plane 1 (Jyy) that of an image that varies only from column to column, plane 2 is Jxy.
#pragma once
#include "common.h"

namespace {

constexpr int T = 32;     // output tile edge
constexpr int NT = 1024;  // threads per workgroup (measured fwd+bwd at 96 px, B = 16: 256 -> 50 us, 512 -> 35 us, 1024 -> 29 us: the passes are latency-bound and there are only 144 tiles)
constexpr int PPT = T * T / NT;   // output pixels per thread

template <int R1, int R2>
struct StTaps {
  float g[2 * R1 + 1];
  float dg[2 * R1 + 1];
  float k[2 * R2 + 1];
};

__device__ __forceinline__ float gray_at(const float* __restrict__ img, int H, int W, int y, int x) {
  if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0.f;
  const size_t hw = (size_t)H * W;
  const float* p = img + (size_t)y * W + x;
  return 0.2989f * p[0] + 0.587f * p[hw] + 0.114f * p[2 * hw];
}

// ---------------------------------------------------------------------------------------------
// Computes the structure tensor (Jxx,Jyy,Jxy) of one image on the tile; 4 pixels per thread.
// LDS use (floats): GW*GW + 2*IW*GW + 2*IW*IW, with the 17-tap H-pass output overlaying the
// (dead by then) gray/A buffers.
template <int R1, int R2>
__device__ __forceinline__ void tile_structure_tensor(const float* __restrict__ img, int H, int W, int y0, int x0,
                                                      const StTaps<R1, R2>& tp, float* lds, float (&J)[PPT][3]) {
  constexpr int R = R1 + R2;
  constexpr int GW = T + 2 * R;    // gray patch edge
  constexpr int IW = T + 2 * R2;   // Ix/Iy region edge
  float* sG = lds;
  float* sA1 = sG + GW * GW;
  float* sA2 = sA1 + IW * GW;
  float* sIx = sA2 + IW * GW;
  float* sIy = sIx + IW * IW;
  float* sQ = lds;  // overlays sG/sA1/sA2: 3*T*IW <= GW*GW + 2*IW*GW
  static_assert(3 * T * IW <= GW * GW + 2 * IW * GW, "overlay");
  const int tid = threadIdx.x;

  __syncthreads();  // previous user of the LDS is done
  for (int i = tid; i < GW * GW; i += NT) {
    const int pr = i / GW, pc = i - pr * GW;
    sG[i] = gray_at(img, H, W, y0 - R + pr, x0 - R + pc);
  }
  __syncthreads();
  // 5-tap pass along H: A1 = dg (x)_H gray, A2 = g (x)_H gray                      utils.py:219,221
  for (int i = tid; i < IW * GW; i += NT) {
    const int ar = i / GW, pc = i - ar * GW;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int t = 0; t <= 2 * R1; ++t) {
      const float v = sG[(ar + t) * GW + pc];
      a1 = fmaf(tp.dg[t], v, a1);
      a2 = fmaf(tp.g[t], v, a2);
    }
    sA1[i] = a1;
    sA2[i] = a2;
  }
  __syncthreads();
  // 5-tap pass along W: Ix = g (x)_W A1, Iy = dg (x)_W A2; zero outside the image      utils.py:220,222
  for (int i = tid; i < IW * IW; i += NT) {
    const int ar = i / IW, ac = i - ar * IW;
    float ix = 0.f, iy = 0.f;
#pragma unroll
    for (int t = 0; t <= 2 * R1; ++t) {
      ix = fmaf(tp.g[t], sA1[ar * GW + ac + t], ix);
      iy = fmaf(tp.dg[t], sA2[ar * GW + ac + t], iy);
    }
    const int y = y0 - R2 + ar, x = x0 - R2 + ac;
    const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    sIx[i] = in ? ix : 0.f;
    sIy[i] = in ? iy : 0.f;
  }
  __syncthreads();
  // (2R2+1)-tap pass along H on the products                                          utils.py:225,227,229
  for (int i = tid; i < T * IW; i += NT) {
    const int qr = i / IW, ac = i - qr * IW;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
    for (int t = 0; t <= 2 * R2; ++t) {
      const float ix = sIx[(qr + t) * IW + ac], iy = sIy[(qr + t) * IW + ac];
      q0 = fmaf(tp.k[t], ix * ix, q0);
      q1 = fmaf(tp.k[t], iy * iy, q1);
      q2 = fmaf(tp.k[t], ix * iy, q2);
    }
    sQ[i] = q0;
    sQ[T * IW + i] = q1;
    sQ[2 * T * IW + i] = q2;
  }
  __syncthreads();
  // pass along W                                                                     utils.py:226,228,230
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int p = tid + j * NT, qr = p >> 5, qc = p & 31;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t <= 2 * R2; ++t) {
      const float kk = tp.k[t];
      s0 = fmaf(kk, sQ[qr * IW + qc + t], s0);
      s1 = fmaf(kk, sQ[T * IW + qr * IW + qc + t], s1);
      s2 = fmaf(kk, sQ[2 * T * IW + qr * IW + qc + t], s2);
    }
    J[j][0] = s0;
    J[j][1] = s1;
    J[j][2] = s2;
  }
}

template <int R1, int R2>
constexpr int st_fwd_lds_floats() {
  constexpr int R = R1 + R2, GW = T + 2 * R, IW = T + 2 * R2;
  return GW * GW + 2 * IW * GW + 2 * IW * IW;
}

// ---------------------------------------------------------------------------------------------
// The pointwise chain on the structure tensors (a1,b1,c1) = (Jxx,Jyy,Jxy) of the SR image and (a2,b2,c2) of its ground truth:
// normalize -> inv(S1)*S2 -> eigenvalues -> clamp -> log -> d.  Every intermediate the loss's analytic gradient reads is kept; a
// caller that only wants d leaves the rest to dead-code elimination.
struct StPoint {
  float n1;                  // 1 / sqrt(det S1 + eps), 1 without normalize
  float ah2, bh2, ch2;       // normalized S2
  float A, Bm, C, D;         // inv(S1)*S2 (up to det S1 = 1)
  float ApB, disc, r;        // trace, discriminant before its clamp, sqrt of the clamped one
  float l1, l2, L1, L2;      // eigenvalues before / after the clamp at 1
  float g1, g2;              // their logs
  float d;                   // the distance
};

__device__ __forceinline__ StPoint st_pointwise(float a1, float b1, float c1, float a2, float b2, float c2, int normalize) {
  const float eps = 1e-12f;
  StPoint p;
  // normalize                                                             utils.py:236-239
  float n1 = 1.f, n2 = 1.f;
  if (normalize) {
    n1 = 1.f / sqrtf(a1 * b1 - c1 * c1 + eps);
    n2 = 1.f / sqrtf(a2 * b2 - c2 * c2 + eps);
  }
  const float ah1 = a1 * n1, bh1 = b1 * n1, ch1 = c1 * n1;
  const float ah2 = a2 * n2, bh2 = b2 * n2, ch2 = c2 * n2;
  // inv(S1)*S2                                                            utils.py:248-251
  const float A = bh1 * ah2 - ch1 * ch2;
  const float Bm = ah1 * bh2 - ch1 * ch2;
  const float C = bh1 * ch2 - ch1 * bh2;
  const float D = ah1 * ch2 - ch1 * ah2;
  // eigenvalues                                                           utils.py:260-265
  const float ApB = A + Bm;
  const float disc = ApB * ApB - 4.f * (A * Bm - C * D);
  const float discc = disc < eps ? eps : disc;           // torch.clamp: NaN stays NaN (a max would return eps)
  const float r = sqrtf(discc);
  const float l1 = 0.5f * (ApB - r), l2 = 0.5f * (ApB + r);
  // distance                                                              utils.py:275-280
  const float L1 = l1 < 1.f ? 1.f : l1, L2 = l2 < 1.f ? 1.f : l2;   // likewise: a NaN eigenvalue keeps d NaN
  const float g1 = logf(L1), g2 = logf(L2);
  const float d = sqrtf(g1 * g1 + g2 * g2 + eps);
  p.n1 = n1;
  p.ah2 = ah2, p.bh2 = bh2, p.ch2 = ch2;
  p.A = A, p.Bm = Bm, p.C = C, p.D = D;
  p.ApB = ApB, p.disc = disc, p.r = r;
  p.l1 = l1, p.l2 = l2, p.L1 = L1, p.L2 = L2;
  p.g1 = g1, p.g2 = g2;
  p.d = d;
  return p;
}

// host: taps exactly like utils.py:194-208 (fp32 exp, fp32 normalisation)
template <int R>
void gaussian_taps(float sigma, float* g, float* dg) {
  const float sigma2 = (float)((double)sigma * (double)sigma + 1e-12);
  const float c = (float)(-0.5 / ((double)sigma * (double)sigma + 1e-12));
  float s = 0.f;
  for (int i = 0; i <= 2 * R; ++i) {
    const float x = (float)(i - R);
    g[i] = expf(c * (x * x));
    s += g[i];
  }
  for (int i = 0; i <= 2 * R; ++i) {
    g[i] /= s;
    if (dg) dg[i] = g[i] * -(float)(i - R) / sigma2;
  }
}

int radius_of(float s) {
  int r = (int)(4.0 * (double)s + 0.5);
  return r < 1 ? 1 : r;
}

template <int R1, int R2>
StTaps<R1, R2> make_taps(float sigma, float rho) {
  StTaps<R1, R2> tp;
  gaussian_taps<R1>(sigma, tp.g, tp.dg);
  gaussian_taps<R2>(rho, tp.k, nullptr);
  return tp;
}

}  // namespace
