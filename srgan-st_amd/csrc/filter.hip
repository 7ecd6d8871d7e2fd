// sst_filter2d: the second-order degradation stage - a K x K correlation of each sample of an fp32 batch
// x [B,3,h,w] with a kernel of its own taken from a TABLE (bank [M,K,K], made and normalised on the host in fp64: Gaussian,
// generalised Gaussian, plateau, sinc, or any the user supplies), then noise (colour or gray, Gaussian or signal-dependent), clamp
// and the 1/255 grid.  Per sample, from its row of flt (8 int32): kernel index (-1: no blur), the fp32 bits of sigma_n and of the
// shot coefficient s_p, the gray flag, the Philox key k0, k1, two zero words.
//
// One workgroup of deg::NT threads per (sample, channel, tile of at most ROWS x COLS pixels).  The tile sits in LDS with its p-wide
// ring, the reflection (torch's `reflect`) resolved on load, in degrade.h's plane layout (odd pitch, weight rows in whole float4s);
// the sample's weights are copied from the bank into LDS once; deg::blur_tile makes the one fp32 FMA chain per pixel in row-major
// order, so a pixel's value does not depend on the tile that produced it.  The pass-through and NaN exits are workgroup-uniform.
#include "degrade.h"
#include <cstdlib>

namespace {

constexpr int COLS = 32;               // tile columns
constexpr int ROWS = 32;               // tile rows at most; the launcher takes fewer while the grid is small (see rows_for)

struct Row {
  int idx, gray;
  float sn, sp;
  uint32_t k0, k1;
};

__device__ __forceinline__ Row load_row(const int* __restrict__ flt, int b) {
  const int4 a = reinterpret_cast<const int4*>(flt)[2 * b], k = reinterpret_cast<const int4*>(flt)[2 * b + 1];
  return {a.x, a.w, __int_as_float(a.y), __int_as_float(a.z), (uint32_t)k.x, (uint32_t)k.y};
}

__global__ __launch_bounds__(deg::NT) void filter2d_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const int* __restrict__ flt, const float* __restrict__ bank, int M, int h,
                                                           int w, int K, int quantise, int TH, int ntx) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const int r0 = ty * TH, nr = min(TH, h - r0), c0 = tx * COLS, nc = min(COLS, w - c0);
  const int64_t plane_off = ((int64_t)b * 3 + c) * h * w;
  const float* __restrict__ img = x + plane_off;
  float* __restrict__ out = y + plane_off;
  const Row q = load_row(flt, b);

  // ---- the workgroup-uniform exits
  const bool bad = q.idx < -1 || q.idx >= M || (q.gray & ~1) != 0 || !(q.sn >= 0.f) || !(q.sp >= 0.f);
  if (bad) {
    for (int i = tid; i < nr * nc; i += deg::NT) out[(int64_t)(r0 + i / nc) * w + c0 + i % nc] = __builtin_nanf("");
    return;
  }
  const bool blur = q.idx >= 0, noisy = q.sn != 0.f || q.sp != 0.f;
  if (!blur && !noisy) {                                         // pass-through: the bits, whatever they are
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(img);
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out);
    for (int i = tid; i < nr * nc; i += deg::NT) {
      const int64_t o = (int64_t)(r0 + i / nc) * w + c0 + i % nc;
      dst[o] = src[o];
    }
    return;
  }

  const deg::Layout L(K, 0, TH, COLS, 0, 0);
  const float* s_blur = reinterpret_cast<const float*>(smem + L.o_a);
  if (blur) {
    const int p = L.p, kp = L.kpitch;
    float* s_k = reinterpret_cast<float*>(smem + L.o_k);
    const float* __restrict__ wsrc = bank + (int64_t)q.idx * K * K;
    for (int i = tid; i < K * kp; i += deg::NT) {
      const int dy = i / kp, dx = i - dy * kp;
      s_k[i] = dx < K ? wsrc[dy * K + dx] : 0.f;
    }
    float* plane = reinterpret_cast<float*>(smem + L.o_plane);
    const int wp = nc + 2 * p;
    for (int i = tid; i < (nr + 2 * p) * wp; i += deg::NT) {     // p < min(h, w): one reflection lands inside
      const int r = i / wp, j = i - r * wp;
      plane[r * L.pitch + j] = img[(int64_t)deg::refl(r0 - p + r, h) * w + deg::refl(c0 - p + j, w)];
    }
    __syncthreads();
    deg::blur_tile(plane, L.pitch, s_k, K, reinterpret_cast<float*>(smem + L.o_a), L.bpitch, nr, nc);
    __syncthreads();
  }

  // ---- noise, clamp, quantise
  const uint32_t e0 = q.gray ? 0u : (uint32_t)c * (uint32_t)(h * w);
  for (int i = tid; i < nr * nc; i += deg::NT) {
    const int rr = i / nc, cc = i - rr * nc, yy = r0 + rr, xx = c0 + cc;
    float v = blur ? s_blur[rr * L.bpitch + cc] : img[(int64_t)yy * w + xx];
    if (noisy) {
      const float z = deg::gauss(e0 + (uint32_t)(yy * w + xx), q.k0, q.k1);
      const float sd = q.sp == 0.f ? q.sn : sqrtf(fmaf(q.sp, fmaxf(v, 0.f), q.sn * q.sn));
      v = fmaf(sd, z, v);
    }
    if (quantise) {
      v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);                   // comparisons keep NaN
      v = rintf(255.f * v) / 255.f;
    }
    out[(int64_t)yy * w + xx] = v;
  }
}

// Tile rows: ROWS, halved (down to 8) while the launch has fewer workgroups than the device has compute units - at the training
// shape (LR 24 x 24, B = 16) 32-row tiles are 48 workgroups on 256 CUs.  Measured there at K = 21 with blur and noise on every
// sample (us per batch): 32 rows 27.3, 12 rows 25.0, 8 rows 23.3, 4 rows 25.8 (below 8 the 20 halo rows of a band outweigh its own).
// SST_FILTER_ROWS (dev switch) fixes it.  A pixel's value does not depend on it.
int rows_for(int B, int h, int w) {
  if (const char* e = sst_env("SST_FILTER_ROWS")) {
    const int r = atoi(e);
    if (r >= 1 && r <= ROWS) return r;
  }
  const int64_t ntx = (w + COLS - 1) / COLS;
  int r = ROWS;
  while (r > 8 && (int64_t)B * 3 * ntx * ((h + r - 1) / r) < 256) r >>= 1;
  return r;
}

}  // namespace

SST_API int sst_filter2d(const float* x, float* y, const int* flt, const float* bank, int M, int B, int h, int w, int K, int quantise,
                         void* stream) {
  SST_REQUIRE(x && y && flt, "sst_filter2d: null pointer");
  SST_REQUIRE(x != y, "sst_filter2d: y == x (a tile reads its neighbours' pixels: out of place only)");
  SST_REQUIRE(M >= 0, "sst_filter2d: bank of %d kernels", M);
  SST_REQUIRE(bank || M == 0, "sst_filter2d: null bank with M = %d", M);
  SST_REQUIRE(B > 0 && B <= 65535, "sst_filter2d: batch %d outside [1, 65535]", B);
  SST_REQUIRE(h > 0 && w > 0 && h <= 8192 && w <= 8192, "sst_filter2d: image %dx%d outside 1..8192", w, h);
  SST_REQUIRE(K >= deg::K_MIN && K <= deg::K_MAX && (K & 1), "sst_filter2d: the window K = %d must be odd and in %d..%d", K, deg::K_MIN,
              deg::K_MAX);
  SST_REQUIRE(M == 0 || K / 2 < (h < w ? h : w),
              "sst_filter2d: the half window %d (K = %d) must be smaller than the image's shorter side (%dx%d)", K / 2, K, w, h);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(flt) & 31) == 0, "sst_filter2d: flt must be 32-byte aligned (rows of 8 int32)");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(bank) & 15) == 0, "sst_filter2d: bank must be 16-byte aligned");
  const int TH = rows_for(B, h, w);
  const int ntx = (w + COLS - 1) / COLS;
  const int64_t ntile = (int64_t)ntx * ((h + TH - 1) / TH);
  SST_REQUIRE(ntile <= 0x7fffffff, "sst_filter2d: %lld tiles per plane", (long long)ntile);
  const int64_t lds = deg::Layout(K, 0, TH, COLS, 0, 0).bytes;
  SST_REQUIRE(lds <= deg::LDS_BUDGET, "sst_filter2d: %lld B of LDS needed > 64 KiB", (long long)lds);
  filter2d_kernel<<<dim3((unsigned)ntile, 3, B), deg::NT, (size_t)lds, sst_stream(stream)>>>(x, y, flt, bank, M, h, w, K, quantise, TH,
                                                                                             ntx);
  SST_LAUNCH_CHECK("filter2d_kernel");
  return SST_OK;
}
