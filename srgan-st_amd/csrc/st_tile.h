// What the structure-tensor family shares: the structure tensor of one 32x32 tile (st_loss.hip, st_maps.hip), and for those two and
// the separable path (st_general.hip) the pointwise distance chain, the two shared parts of its gradient, the stores of the maps
// and of d(sr), the host's taps, the list of tile builds and the grid.  Every translation unit that includes this gets its own
// copy (unnamed namespace).
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
#include <type_traits>

#include "common.h"

namespace {

constexpr int T = 32;     // output tile edge, of the tile kernels and of every pass of the general path
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

// ---------------------------------------------------------------------------------------------
// The analytic gradient of d wrt (a1,b1,c1), unit upstream, in the two parts every forward shares.  Between them each kernel forms
// dA, dB, dC, dD = d d / d (A, Bm, C, D) itself, from its own discriminant (st_general.hip says why its differs).
struct StEigGrad { float dl12, ddisc; };   // d d / d l1 + d d / d l2 (twice d d / d ApB through the eigenvalues' mean), d d / d disc

// head: given the eigenvalue-side values the kernel uses (l before / L after the clamp at 1, g their logs, r = sqrt of the clamped disc)
__device__ __forceinline__ StEigGrad st_grad_eigen(float d, float l1, float l2, float L1, float L2, float g1, float g2, float disc, float r) {
  const float dq = 0.5f / d;
  const float dl1 = (l1 >= 1.f) ? dq * 2.f * g1 / L1 : 0.f;
  const float dl2 = (l2 >= 1.f) ? dq * 2.f * g2 / L2 : 0.f;
  const float dr = 0.5f * (dl2 - dl1);
  return {dl1 + dl2, (disc >= 1e-12f) ? dr / (2.f * r) : 0.f};
}

__device__ __forceinline__ void store_planes(float* __restrict__ out, size_t o, size_t hw, float v0, float v1, float v2) {
  out[o] = v0;
  out[o + hw] = v1;
  out[o + 2 * hw] = v2;
}

// tail: (dA, dB, dC, dD) -> through inv(S1)*S2 and the normalize correction -> gS[o + {0,1,2} hw] = d d / d (a1, b1, c1)
__device__ __forceinline__ void st_grad_store(float* __restrict__ gS, size_t o, size_t hw, float dA, float dB, float dC, float dD,
                                              const StPoint& pt, float a1, float b1, float c1, int normalize) {
  const float n1 = pt.n1, ah2 = pt.ah2, bh2 = pt.bh2, ch2 = pt.ch2;
  const float dah = dB * bh2 + dD * ch2;
  const float dbh = dA * ah2 + dC * ch2;
  const float dch = -(dA + dB) * ch2 - dC * bh2 - dD * ah2;
  float ga = dah * n1, gb = dbh * n1, gc = dch * n1;
  if (normalize) {
    const float dn = a1 * dah + b1 * dbh + c1 * dch;
    const float ddet = dn * (-0.5f * n1 * n1 * n1);
    ga += ddet * b1;
    gb += ddet * a1;
    gc -= 2.f * ddet * c1;
  }
  store_planes(gS, o, hw, ga, gb, gc);
}

// d(sr)[o + c hw] (+)= gray_w[c] * v (+ pv[c], a per-channel pixel term, where pv is not null): a gray image's gradient as RGB
__device__ __forceinline__ void store_gray_grad(float* __restrict__ dsr, size_t o, size_t hw, float v, int accumulate, const float* pv) {
  // formed inside each branch: the product of an accumulating store contracts with its sum, as it did before the stores were one
  const auto rgb = [&](int c, float w) { return pv ? w * v + pv[c] : w * v; };
  if (accumulate) {
    dsr[o] += rgb(0, 0.2989f);
    dsr[o + hw] += rgb(1, 0.587f);
    dsr[o + 2 * hw] += rgb(2, 0.114f);
  } else {
    store_planes(dsr, o, hw, rgb(0, 0.2989f), rgb(1, 0.587f), rgb(2, 0.114f));
  }
}

// ---------------------------------------------------------------------------------------------
// The maps (sst_st_maps, sst_st_general_maps): each output optional, a null pointer = neither computed nor stored.
struct StMapsOut {
  float* Sx;
  float* Sgt;
  float* Fx;
  float* Fgt;
  float* d;
  float* tile_sums;
  __device__ bool want_d() const { return d || tile_sums; }
};

// (t, c2, s2) of one structure tensor
__device__ __forceinline__ void store_features(float* __restrict__ out, size_t o, size_t hw, float jxx, float jyy, float jxy) {
  const float t = jxx + jyy;
  const float den = t + 1e-12f;
  store_planes(out, o, hw, t, (jxx - jyy) / den, 2.f * jxy / den);
}

// One pixel (px within image b's planes) of every map asked for, from J1 = S(x), J2 = S(gt); its d, where wanted, is added to lsum
__device__ __forceinline__ void maps_pixel(const StMapsOut& out, int b, size_t px, size_t hw, const float (&J1)[3], const float (&J2)[3],
                                           int normalize, float& lsum) {
  const size_t o = (size_t)b * 3 * hw + px;
  if (out.Sx) store_planes(out.Sx, o, hw, J1[0], J1[1], J1[2]);
  if (out.Sgt) store_planes(out.Sgt, o, hw, J2[0], J2[1], J2[2]);
  if (out.Fx) store_features(out.Fx, o, hw, J1[0], J1[1], J1[2]);
  if (out.Fgt) store_features(out.Fgt, o, hw, J2[0], J2[1], J2[2]);
  if (out.want_d()) {
    const float d = st_pointwise(J1[0], J1[1], J1[2], J2[0], J2[1], J2[2], normalize).d;
    if (out.d) out.d[(size_t)b * hw + px] = d;
    lsum += d;
  }
}

// tile_sums[b][tile] = the workgroup's sum of d; the branch is uniform: every thread of every workgroup takes the same side
template <int NTHREADS>
__device__ __forceinline__ void maps_tile_sum(const StMapsOut& out, int b, float lsum, float* red) {
  if (!out.tile_sums) return;
  const float bsum = block_sum<NTHREADS>(lsum, red);
  if (threadIdx.x == 0) out.tile_sums[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = bsum;
}

// ------------------------------------------------------------------------------------------ host
// What both maps entries ask of their arguments besides their own pointers; `who` is the entry's name.
int maps_args_ok(const char* who, bool shape_ok, int B, int H, int W, const float* gt, const StMapsOut& out) {
  SST_REQUIRE(shape_ok, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
  SST_REQUIRE(out.Sx || out.Sgt || out.Fx || out.Fgt || out.d || out.tile_sums, "%s: no output requested", who);
  SST_REQUIRE(gt || !out.Sgt, "%s: Sgt needs gt", who);
  SST_REQUIRE(gt || !out.Fgt, "%s: Fgt needs gt", who);
  SST_REQUIRE(gt || !out.d, "%s: d needs gt (the distance is between two images)", who);
  SST_REQUIRE(gt || !out.tile_sums, "%s: tile_sums cannot be computed without gt (they are sums of d)", who);
  return SST_OK;
}

// One workgroup per 32 x 32 tile, in every kernel of the family.  The grid's z carries the images (twice B on the general path, so
// its entries bound B by 32767 where the tile entries take 65535), its y the tile rows.
dim3 tiles_grid(int H, int W, int z) { return dim3((W + T - 1) / T, (H + T - 1) / T, z); }
int64_t tiles_of(int B, int H, int W) { return (int64_t)B * ((H + T - 1) / T) * ((W + T - 1) / T); }
bool shape_ok(int B, int H, int W, int max_b) { return B > 0 && H > 0 && W > 0 && B <= max_b && (H + T - 1) / T <= 65535; }

// The tile builds: f(R1, R2) with the radii as compile-time values (std::integral_constant) for the build (r1, r2) selects ->
// whether there is one.
template <class F>
bool with_tile_build(int r1, int r2, F&& f) {
  if (r1 == 2 && r2 == 8) return f(std::integral_constant<int, 2>{}, std::integral_constant<int, 8>{}), true;
  if (r1 == 4 && r2 == 10) return f(std::integral_constant<int, 4>{}, std::integral_constant<int, 10>{}), true;
  return false;
}

// taps exactly like utils.py:194-208 (fp32 exp, fp32 normalisation)
void gaussian_taps(float sigma, int R, float* g, float* dg) {
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
  gaussian_taps(sigma, R1, tp.g, tp.dg);
  gaussian_taps(rho, R2, tp.k, nullptr);
  return tp;
}

}  // namespace
