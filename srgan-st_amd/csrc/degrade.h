// The blind-SR degradation stage, the device code shared by its two entries: sst_gather_crops_degraded
// (data.hip: crop, transform, conversion, then this) and sst_degrade (degrade.hip: an fp32 batch, then this).  Per sample
//   lr = quantise( clamp( bicubic_down( x (*) k ) + n ) ),   k an anisotropic Gaussian, n Gaussian noise, both from the sample's deg row
// deg row (8 int32, 32 bytes): the fp32 bits of qa, qb, qc, sigma_n, then the Philox key k0, k1, then two zero words.  qa < 0: no blur.
//
// One workgroup owns one TILE of one image plane: noy <= ROWS_MAX LR rows by nox LR columns.  Its taps name the blur rows
// [r0, r0 + nr) and blur columns [c0, c0 + nc); the caller fills the fp32 PLANE, (nr + 2p) rows of `pitch` floats, with the pixels
// those name and their reflected halo:  plane[r][j] = x[refl(r0 - p + r)][refl(c0 - p + j)],  j < nc + 2p  (torch's `reflect`).
// Then, each with the term order of the issue, so that a result does not depend on the tile that produced it:
//   weights   w = expf(-(qa dx^2 + qb dx dy + qc dy^2)), fp64 sum in row-major order by one thread, k = fl32(w / sum)   (LDS, K rows)
//   blur      one fp32 FMA chain per pixel in row-major order; a thread owns 4 adjacent pixels of a row and slides over the plane
//             row: one float4 of weights and 4 plane values feed 16 FMAs; 32 lanes take 8 pixel groups x 4 rows and the pitch is
//             odd: no bank conflict
//   vertical  V[rr][j] = sum_ty B[iy[ty]][j] * wy[ty]      horizontal  d = sum_tx V[rr][ix[tx]] * wx[tx]     (gather_crops_kernel's)
//   noise     Philox4x32-10, counter (e, 0, 0, 0), key (k0, k1), e the element's index in the sample's LR; Box-Muller on x0, x1
//   quantise  a degraded sample is clamped to [0, 1]; rintf(255 v) / 255 unless the launch asks for the raw value
// A table entry outside the tile is clamped into it (no read outside LDS); the callers refuse a tile larger than the host sized.
#pragma once
#include "common.h"

namespace deg {

constexpr int NT = 256;             // (1024 threads were measured: no faster at K = 21, slower at K = 7)
constexpr int K_MIN = 3, K_MAX = 21;
constexpr int ROWS_MAX = 2;            // LR rows of one workgroup at most.  Measured at B = 16, S = 96, x4 (us per batch, K = 7 / 21): 2 rows 23.7 /
                                       // 78.3, 4 rows 30.0 / 98.7 - fewer redundant blur rows (1.75x against 2.5x) do not pay for half the workgroups
constexpr int TILE_COLS = 16;          // LR columns of one workgroup of sst_degrade (device_data.DEGRADE_TILE_COLS)
constexpr int64_t LDS_BUDGET = 64 * 1024;

struct Params {
  float qa, qb, qc, sn;
  uint32_t k0, k1;
  __device__ bool blur() const { return !(qa < 0.f); }
  __device__ bool noisy() const { return !(sn == 0.f); }
};

__device__ __forceinline__ Params load_params(const int* __restrict__ deg, int b) {
  const int4 a = reinterpret_cast<const int4*>(deg)[2 * b], k = reinterpret_cast<const int4*>(deg)[2 * b + 1];
  return {__int_as_float(a.x), __int_as_float(a.y), __int_as_float(a.z), __int_as_float(a.w), (uint32_t)k.x, (uint32_t)k.y};
}

__host__ __device__ inline int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// The LDS of one workgroup, in bytes from the start: the fp64 sum, the K rows of weights, V, the plane, then region A = the blurred tile,
// which the crops kernel also uses for its staged bytes (dead once the plane is filled), then `tail` bytes of the caller's own.
struct Layout {
  int p, pitch, bpitch, kpitch, nr_max, nc_max;
  int64_t o_k, o_v, o_plane, o_a, o_tail, bytes;
  __host__ __device__ Layout(int K, int rows, int nr_max_, int nc_max_, int64_t raw_bytes, int64_t tail) {
    p = K >> 1, nr_max = nr_max_, nc_max = nc_max_;
    bpitch = (nc_max + 3) & ~3;
    pitch = (bpitch + 2 * p + 4) | 1;                    // the sliding blur reads up to bpitch + 2p + 3; odd: see blur_tile
    kpitch = (K + 3) & ~3;                               // a weight row: whole float4s, the tail zero
    o_k = 16;
    o_v = o_k + (int64_t)K * kpitch * 4;
    o_plane = o_v + (((int64_t)rows * nc_max * 4 + 15) & ~15);
    o_a = o_plane + ((((int64_t)(nr_max + 2 * p) * pitch + 8) * 4 + 15) & ~15);
    const int64_t blur_bytes = (int64_t)nr_max * bpitch * 4;
    o_tail = o_a + (((raw_bytes > blur_bytes ? raw_bytes : blur_bytes) + 15) & ~15);
    bytes = o_tail + tail;
  }
};

// ---- weights, in three steps so that the one-thread fp64 sum can run beside the other threads' plane fill.  s_k: K rows of
// kpitch = (K + 3) & ~3 floats, the tail of a row zero, so that the blur reads a row in whole float4s
__device__ __forceinline__ void weights_raw(float* __restrict__ s_k, const Params& q, int K) {
  const int p = K >> 1, kp = (K + 3) & ~3;
  for (int i = threadIdx.x; i < K * kp; i += NT) {
    const float dy = (float)(i / kp - p), dx = (float)(i % kp - p);
    s_k[i] = i % kp < K ? expf(-(q.qa * dx * dx + q.qb * dx * dy + q.qc * dy * dy)) : 0.f;
  }
}
__device__ __forceinline__ void weights_sum(const float* __restrict__ s_k, double* __restrict__ s_sum, int K) {   // ONE thread
  static_assert(K_MAX <= 24, "weights_sum reads a weight row as six float4s");
  const int kp = (K + 3) & ~3;
  double s = 0.0;
  for (int dy = 0; dy < K; ++dy) {                               // a row's loads together, then its adds in order (441 dependent
    const float4* row = reinterpret_cast<const float4*>(s_k + dy * kp);   // load-then-add steps measured 4 us more per launch at K = 21)
    float4 v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = row[j];                   // past a short row: other LDS of the workgroup, read and not added
#pragma unroll
    for (int j = 0; j < 6; ++j)
      if (4 * j < kp) s += (double)v[j].x, s += (double)v[j].y, s += (double)v[j].z, s += (double)v[j].w;   // the zero tail adds nothing
  }
  *s_sum = s;
}
__device__ __forceinline__ void weights_norm(float* __restrict__ s_k, const double* __restrict__ s_sum, int K) {
  const int kp = (K + 3) & ~3;
  const double sum = *s_sum;
  const bool ok = sum > 0.0 && sum < __builtin_huge_val();       // false for NaN too: the sample's LR is then NaN
  for (int i = threadIdx.x; i < K * kp; i += NT)
    if (i % kp < K) s_k[i] = ok ? (float)((double)s_k[i] / sum) : __builtin_nanf("");
}

// ---- blur: out[row][x] = sum_{dy,dx} k[dy][dx] * plane[row + dy][x + dx], row < nr, x < nc
__device__ __forceinline__ void blur_tile(const float* __restrict__ plane, int pitch, const float* __restrict__ s_k, int K,
                                          float* __restrict__ out, int bpitch, int nr, int nc) {
  const int ngx = (nc + 3) >> 2, ngx8 = (ngx + 7) >> 3, nr4 = (nr + 3) >> 2, kp = (K + 3) & ~3;
  for (int it = threadIdx.x; it < nr4 * ngx8 * 32; it += NT) {
    const int rest = it >> 5;
    const int xg = (rest % ngx8) * 8 + (it & 7), row = (rest / ngx8) * 4 + ((it >> 3) & 3);
    if (xg >= ngx || row >= nr) continue;
    const int x0 = xg * 4;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int dy = 0; dy < K; ++dy) {
      const float* src = plane + (row + dy) * pitch + x0;
      const float4* kr = reinterpret_cast<const float4*>(s_k + dy * kp);
      float d0 = src[0], d1 = src[1], d2 = src[2], d3 = src[3];
      for (int dx = 0; dx < K; dx += 4) {                        // all eight loads first; the tail's steps are skipped, not zeroed
        const float4 w = kr[dx >> 2];
        const float n0 = src[dx + 4], n1 = src[dx + 5], n2 = src[dx + 6], n3 = src[dx + 7];
        a0 = fmaf(w.x, d0, a0), a1 = fmaf(w.x, d1, a1), a2 = fmaf(w.x, d2, a2), a3 = fmaf(w.x, d3, a3);
        if (dx + 1 < K) a0 = fmaf(w.y, d1, a0), a1 = fmaf(w.y, d2, a1), a2 = fmaf(w.y, d3, a2), a3 = fmaf(w.y, n0, a3);
        if (dx + 2 < K) a0 = fmaf(w.z, d2, a0), a1 = fmaf(w.z, d3, a1), a2 = fmaf(w.z, n0, a2), a3 = fmaf(w.z, n1, a3);
        if (dx + 3 < K) a0 = fmaf(w.w, d3, a0), a1 = fmaf(w.w, n0, a1), a2 = fmaf(w.w, n1, a2), a3 = fmaf(w.w, n2, a3);
        d0 = n0, d1 = n1, d2 = n2, d3 = n3;
      }
    }
    float* o = out + row * bpitch + x0;                          // bpitch is a multiple of 4: the whole group is inside the row
    o[0] = a0, o[1] = a1, o[2] = a2, o[3] = a3;
  }
}

// ---- noise: one standard normal per LR element
__device__ __forceinline__ float gauss(uint32_t e, uint32_t k0, uint32_t k1) {
  uint32_t c0 = e, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  const float u1 = fmaf((float)(c0 >> 8), 0x1p-24f, 0x1p-25f), u2 = fmaf((float)(c1 >> 8), 0x1p-24f, 0x1p-25f);
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);              // cos(2 pi u2), the argument reduced exactly
}

// The geometry of one tile (all workgroup-uniform)
struct Tile {
  int r0, nr, c0, nc;              // blur rows / columns
  int oy0, noy, ox0, nox;          // LR rows / columns owned
};

// ---- everything after the plane fill.  Call from ALL threads, after weights_raw (when q.blur()) and a barrier behind the fill and
// the weights_sum.  lr_plane: the [oh, ow] LR plane of this (sample, channel); e0: the element index of its first element.
__device__ __forceinline__ void finish_tile(unsigned char* __restrict__ smem, const Layout& L, const Tile& t, const Params& q, int K,
                                            int quantise, float* __restrict__ lr_plane, uint32_t e0, const float* __restrict__ wy,
                                            const int* __restrict__ iy, const float* __restrict__ wx, const int* __restrict__ ix,
                                            int ow, int Ty, int Tx) {
  float* s_k = reinterpret_cast<float*>(smem + L.o_k);
  float* s_v = reinterpret_cast<float*>(smem + L.o_v);
  const float* plane = reinterpret_cast<const float*>(smem + L.o_plane);
  float* s_blur = reinterpret_cast<float*>(smem + L.o_a);
  const float* src = plane + L.p * L.pitch + L.p;                // no blur: the tile itself
  int sp = L.pitch;
  if (q.blur()) {
    weights_norm(s_k, reinterpret_cast<const double*>(smem), K);
    __syncthreads();
    blur_tile(plane, L.pitch, s_k, K, s_blur, L.bpitch, t.nr, t.nc);
    __syncthreads();
    src = s_blur, sp = L.bpitch;
  }
  // vertical pass (gather_crops_kernel's term order: v += in * wy in table order)
  for (int i = threadIdx.x; i < t.noy * t.nc; i += NT) {
    const int rr = i / t.nc, j = i - rr * t.nc;
    const float* wrow = wy + (int64_t)(t.oy0 + rr) * Ty;
    const int* irow = iy + (int64_t)(t.oy0 + rr) * Ty;
    float v = 0.f;
    for (int ty = 0; ty < Ty; ++ty) {
      const int r = min(max(irow[ty], t.r0), t.r0 + t.nr - 1) - t.r0;
      v = fmaf(src[r * sp + j], wrow[ty], v);
    }
    s_v[rr * t.nc + j] = v;
  }
  __syncthreads();
  // horizontal pass, noise, quantise
  const bool degraded = q.blur() || q.noisy();
  for (int i = threadIdx.x; i < t.noy * t.nox; i += NT) {
    const int rr = i / t.nox, ox = t.ox0 + (i - rr * t.nox), oy = t.oy0 + rr;
    float v = 0.f;
    for (int tx = 0; tx < Tx; ++tx) {
      const int x = min(max(ix[(int64_t)ox * Tx + tx], t.c0), t.c0 + t.nc - 1) - t.c0;
      v = fmaf(s_v[rr * t.nc + x], wx[(int64_t)ox * Tx + tx], v);
    }
    if (q.noisy()) v = fmaf(q.sn, gauss(e0 + (uint32_t)(oy * ow + ox), q.k0, q.k1), v);
    if (quantise) {
      if (degraded) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);     // comparisons keep NaN
      v = rintf(255.f * v) / 255.f;
    }
    lr_plane[(int64_t)oy * ow + ox] = v;
  }
}

// The rows [lo, hi] that the taps of LR rows [oy0, oy0 + noy) name; false when one lies outside [0, n)
__device__ __forceinline__ bool tap_rows(const int* __restrict__ iy, int Ty, int oy0, int noy, int n, int& lo, int& hi) {
  bool ok = true;
  lo = n, hi = -1;
  for (int k = 0; k < noy * Ty; ++k) {
    const int r = iy[(int64_t)oy0 * Ty + k];
    ok = ok && r >= 0 && r < n;
    lo = min(lo, r), hi = max(hi, r);
  }
  return ok && hi >= lo;
}

__device__ __forceinline__ void fill_nan(float* __restrict__ lr_plane, const Tile& t, int ow) {
  for (int i = threadIdx.x; i < t.noy * t.nox; i += NT)
    lr_plane[(int64_t)(t.oy0 + i / t.nox) * ow + t.ox0 + i % t.nox] = __builtin_nanf("");
}

}  // namespace deg
