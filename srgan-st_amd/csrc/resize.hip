// sst_rescale: the random resize round trip of the second-order degradation.  Per sample of an fp32 batch
// x [B,3,h,w]: resample to an intermediate size (hi, wi) of its own with mode m1, add noise 2 THERE (sst_filter2d's rule, element
// index in the intermediate image), resample back to (h, w) with mode m2, clamp and the 1/255 grid.  Input and output geometry are
// the launch's; the intermediate image exists only in LDS.  Per sample, from its row of `rows` (8 int32): hi, wi (0, 0: no resize),
// the fp32 bits of sigma_n and of the shot coefficient s_p, the Philox key k0, k1, then m1 | m2 << 2 | gray << 4 (modes: 0 area,
// 1 bilinear, 2 bicubic), then a zero word.
//
// One workgroup of deg::NT threads per (sample, channel, output tile of at most ROWS x COLS pixels).  The taps of every axis are made
// in integer arithmetic (no tap depends on a floating-point floor) and kept as tables in LDS: for an index its first tap, its tap
// count and up to five weights.  Phase 1 computes the intermediate pixels that the tile's back-resize taps name - at a ratio of at
// most 2 no more than (2 ROWS + 4) x (2 COLS + 4) - straight from global memory, each by the one fmaf chain of the model, so that an
// intermediate pixel has the same bits whichever workgroup needs it, and adds the noise.  Phase 2 makes the tile from LDS.  The
// pass-through, NaN and no-resize exits are workgroup-uniform and come before any LDS use.
#include "degrade.h"
#include <cstdlib>

namespace {

constexpr int COLS = 32;               // tile columns
constexpr int ROWS = 32;               // tile rows at most; the launcher takes fewer while the grid is small (see rows_for)
constexpr int TAPS = 5;                // area at n_in <= 4 n_out: at most 5 taps; bilinear 2, bicubic 4
constexpr int RATIO = 2;               // hi <= RATIO h: what bounds the intermediate pixels of a tile
constexpr int MIN_DIV = 4;             // RATIO's counterpart downwards: MIN_DIV hi >= h
constexpr int NIX = RATIO * COLS + 4;  // intermediate columns of a tile at most
constexpr int PITCH = NIX | 1;         // odd: rows of the intermediate tile start on different banks

__host__ __device__ constexpr int niy_for(int TH) { return RATIO * TH + 4; }

struct Row {
  int hi, wi, m1, m2, gray, high;
  float sn, sp;
  uint32_t k0, k1;
};

__device__ __forceinline__ Row load_row(const int* __restrict__ rows, int b) {
  const int4 a = reinterpret_cast<const int4*>(rows)[2 * b], k = reinterpret_cast<const int4*>(rows)[2 * b + 1];
  return {a.x, a.y, k.z & 3, (k.z >> 2) & 3, (k.z >> 4) & 1, k.z >> 5, __int_as_float(a.z), __int_as_float(a.w), (uint32_t)k.x, (uint32_t)k.y};
}

// ---- one axis, n_in -> n_out, output index i: the taps are clamp(base + k, 0, n_in - 1), k < n, with weights w[k]
__device__ __forceinline__ int floor_div(int num, int den) { return num >= 0 ? num / den : -((den - 1 - num) / den); }

struct Frac {
  int f;
  float t;
};
__device__ __forceinline__ Frac frac(int i, int n_in, int n_out) {       // the source coordinate (i + 0.5) n_in / n_out - 0.5 = f + t
  const int num = (2 * i + 1) * n_in - n_out, den = 2 * n_out;             // both below 2^24 after the floor: t is rounded once
  const int f = floor_div(num, den);
  return {f, (float)(num - f * den) / (float)den};
}

// the first and the last tap of output index i, clamped
__device__ __forceinline__ void tap_span(int mode, int i, int n_in, int n_out, int& lo, int& hi) {
  if (mode == 0) {
    lo = (i * n_in) / n_out, hi = ((i + 1) * n_in + n_out - 1) / n_out - 1;
    return;
  }
  const int f = floor_div((2 * i + 1) * n_in - n_out, 2 * n_out);
  if (mode == 1) {
    const int g = max(f, 0);
    lo = min(g, n_in - 1), hi = min(g + 1, n_in - 1);
  } else {
    lo = min(max(f - 1, 0), n_in - 1), hi = min(max(f + 2, 0), n_in - 1);
  }
}

// torch's cubic convolution coefficients, A = -0.75
__device__ __forceinline__ float cc1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.f; }
__device__ __forceinline__ float cc2(float x) { return ((-0.75f * x + 3.75f) * x - 6.f) * x + 3.f; }

// A table of L entries in LDS: base[L], n[L], then TAPS rows of L weights (an unused weight is never read)
struct Table {
  int* base;
  int* n;
  float* w;
  int L;
  __device__ Table(float* p, int L_) : base(reinterpret_cast<int*>(p)), n(reinterpret_cast<int*>(p) + L_), w(p + 2 * L_), L(L_) {}
  __host__ __device__ static constexpr int floats(int L_) { return (2 + TAPS) * L_; }
};

__device__ __forceinline__ void make_taps(const Table& T, int slot, int mode, int i, int n_in, int n_out) {
  const int L = T.L;
  if (mode == 0) {
    const int a = (i * n_in) / n_out, b = ((i + 1) * n_in + n_out - 1) / n_out;
    const float wgt = 1.f / (float)(b - a);
    T.base[slot] = a, T.n[slot] = min(b - a, TAPS);
#pragma unroll
    for (int k = 0; k < TAPS; ++k) T.w[k * L + slot] = wgt;
    return;
  }
  Frac q = frac(i, n_in, n_out);
  if (mode == 1) {
    if (q.f < 0) q.f = 0, q.t = 0.f;
    T.base[slot] = q.f, T.n[slot] = 2;
    T.w[slot] = 1.f - q.t, T.w[L + slot] = q.t;
  } else {
    T.base[slot] = q.f - 1, T.n[slot] = 4;
    T.w[slot] = cc2(q.t + 1.f), T.w[L + slot] = cc1(q.t), T.w[2 * L + slot] = cc1(1.f - q.t), T.w[3 * L + slot] = cc2(2.f - q.t);
  }
}

__device__ __forceinline__ float finish(float v, int quantise) {
  if (quantise) {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);                     // comparisons keep NaN
    v = rintf(255.f * v) / 255.f;
  }
  return v;
}

__global__ __launch_bounds__(deg::NT) void rescale_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const int* __restrict__ rows, int h, int w, int quantise, int TH, int ntx) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const int r0 = ty * TH, nr = min(TH, h - r0), c0 = tx * COLS, nc = min(COLS, w - c0);
  const int64_t plane_off = ((int64_t)b * 3 + c) * h * w;
  const float* __restrict__ img = x + plane_off;
  float* __restrict__ out = y + plane_off;
  const Row q = load_row(rows, b);

  // ---- the workgroup-uniform exits
  const bool sized = q.hi != 0 || q.wi != 0;
  const bool bad = q.hi < 0 || q.wi < 0 || (q.hi == 0) != (q.wi == 0) || q.m1 == 3 || q.m2 == 3 || q.high != 0 || !(q.sn >= 0.f) ||
                   !(q.sp >= 0.f) ||
                   (sized && ((int64_t)MIN_DIV * q.hi < h || q.hi > RATIO * h || (int64_t)MIN_DIV * q.wi < w || q.wi > RATIO * w));
  if (bad) {
    for (int i = tid; i < nr * nc; i += deg::NT) out[(int64_t)(r0 + i / nc) * w + c0 + i % nc] = __builtin_nanf("");
    return;
  }
  const bool noisy = q.sn != 0.f || q.sp != 0.f;
  if (!sized && !noisy) {                                        // pass-through: the bits, whatever they are
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(img);
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out);
    for (int i = tid; i < nr * nc; i += deg::NT) {
      const int64_t o = (int64_t)(r0 + i / nc) * w + c0 + i % nc;
      dst[o] = src[o];
    }
    return;
  }
  if (!sized) {                                                  // noise at the image's own size: u = x, sst_filter2d's noise pass
    const uint32_t e0 = q.gray ? 0u : (uint32_t)c * (uint32_t)(h * w);
    for (int i = tid; i < nr * nc; i += deg::NT) {
      const int rr = i / nc, yy = r0 + rr, xx = c0 + (i - rr * nc);
      float v = img[(int64_t)yy * w + xx];
      const float z = deg::gauss(e0 + (uint32_t)(yy * w + xx), q.k0, q.k1);
      const float sd = q.sp == 0.f ? q.sn : sqrtf(fmaf(q.sp, fmaxf(v, 0.f), q.sn * q.sn));
      v = fmaf(sd, z, v);
      out[(int64_t)yy * w + xx] = finish(v, quantise);
    }
    return;
  }

  // ---- the intermediate pixels that this tile's back-resize names: rows [Y0, Y1], columns [X0, X1]
  const int hi = q.hi, wi = q.wi;
  int Y0, Y1, X0, X1, unused;
  tap_span(q.m2, r0, hi, h, Y0, unused);
  tap_span(q.m2, r0 + nr - 1, hi, h, unused, Y1);
  tap_span(q.m2, c0, wi, w, X0, unused);
  tap_span(q.m2, c0 + nc - 1, wi, w, unused, X1);
  const int nyi = Y1 - Y0 + 1, nxi = X1 - X0 + 1, NIY = niy_for(TH);
  if (nyi < 1 || nxi < 1 || nyi > NIY || nxi > NIX) {            // cannot be at ratios within [1 / MIN_DIV, RATIO]: no write outside LDS
    for (int i = tid; i < nr * nc; i += deg::NT) out[(int64_t)(r0 + i / nc) * w + c0 + i % nc] = __builtin_nanf("");
    return;
  }

  float* s_u = lds;                                              // [NIY][PITCH]
  const Table t_iy(s_u + NIY * PITCH, NIY), t_ix(t_iy.w + TAPS * NIY, NIX), t_oy(t_ix.w + TAPS * NIX, TH), t_ox(t_oy.w + TAPS * TH, COLS);
  for (int i = tid; i < nyi + nxi + nr + nc; i += deg::NT) {
    if (i < nyi) make_taps(t_iy, i, q.m1, Y0 + i, h, hi);
    else if (i < nyi + nxi) make_taps(t_ix, i - nyi, q.m1, X0 + i - nyi, w, wi);
    else if (i < nyi + nxi + nr) make_taps(t_oy, i - nyi - nxi, q.m2, r0 + i - nyi - nxi, hi, h);
    else make_taps(t_ox, i - nyi - nxi - nr, q.m2, c0 + i - nyi - nxi - nr, wi, w);
  }
  __syncthreads();

  // ---- phase 1: u[Y][X] = sum_j wy[j] (sum_i wx[i] x[iy_j][ix_i]), then the noise at the intermediate resolution
  const uint32_t e0 = q.gray ? 0u : (uint32_t)c * (uint32_t)(hi * wi);
  for (int i = tid; i < nyi * nxi; i += deg::NT) {
    const int ry = i / nxi, rx = i - ry * nxi;
    const int by = t_iy.base[ry], ny = t_iy.n[ry], bx = t_ix.base[rx], nx = t_ix.n[rx];
    float v = 0.f;
    for (int j = 0; j < ny; ++j) {
      const float* __restrict__ src = img + (int64_t)min(max(by + j, 0), h - 1) * w;
      float r = 0.f;
      for (int k = 0; k < nx; ++k) r = fmaf(t_ix.w[k * NIX + rx], src[min(max(bx + k, 0), w - 1)], r);
      v = fmaf(t_iy.w[j * NIY + ry], r, v);
    }
    if (noisy) {
      const float z = deg::gauss(e0 + (uint32_t)((Y0 + ry) * wi + X0 + rx), q.k0, q.k1);
      const float sd = q.sp == 0.f ? q.sn : sqrtf(fmaf(q.sp, fmaxf(v, 0.f), q.sn * q.sn));
      v = fmaf(sd, z, v);
    }
    s_u[ry * PITCH + rx] = v;
  }
  __syncthreads();

  // ---- phase 2: back to (h, w) by the same rule on u, clamp, quantise
  for (int i = tid; i < nr * nc; i += deg::NT) {
    const int rr = i / nc, cc = i - rr * nc;
    const int by = t_oy.base[rr], ny = t_oy.n[rr], bx = t_ox.base[cc], nx = t_ox.n[cc];
    float v = 0.f;
    for (int j = 0; j < ny; ++j) {
      const float* src = s_u + (min(max(by + j, Y0), Y1) - Y0) * PITCH;        // (a tap is inside [Y0, Y1] x [X0, X1]: the clamp is
      float r = 0.f;                                                            // the model's at the image's edge, and holds LDS reads in)
      for (int k = 0; k < nx; ++k) r = fmaf(t_ox.w[k * COLS + cc], src[min(max(bx + k, X0), X1) - X0], r);
      v = fmaf(t_oy.w[j * TH + rr], r, v);
    }
    out[(int64_t)(r0 + rr) * w + c0 + cc] = finish(v, quantise);
  }
}

int64_t lds_bytes(int TH) {
  const int NIY = niy_for(TH);
  return 4 * ((int64_t)NIY * PITCH + Table::floats(NIY) + Table::floats(NIX) + Table::floats(TH) + Table::floats(COLS));
}

// Tile rows: sst_filter2d's rule - ROWS, halved (down to 8) while the launch has fewer workgroups than the device has compute units.
// SST_RESIZE_ROWS (dev switch) fixes it.  A pixel's value does not depend on it.
int rows_for(int B, int h, int w) {
  if (const char* e = sst_env("SST_RESIZE_ROWS")) {
    const int r = atoi(e);
    if (r >= 1 && r <= ROWS) return r;
  }
  const int64_t ntx = (w + COLS - 1) / COLS;
  int r = ROWS;
  while (r > 8 && (int64_t)B * 3 * ntx * ((h + r - 1) / r) < 256) r >>= 1;
  return r;
}

}  // namespace

SST_API int sst_rescale(const float* x, float* y, const int* rows, int B, int h, int w, int quantise, void* stream) {
  SST_REQUIRE(x && y && rows, "sst_rescale: null pointer");
  SST_REQUIRE(x != y, "sst_rescale: y == x (a tile reads its neighbours' pixels: out of place only)");
  SST_REQUIRE(B > 0 && B <= 65535, "sst_rescale: batch %d outside [1, 65535]", B);
  SST_REQUIRE(h > 0 && w > 0 && h <= 8192 && w <= 8192, "sst_rescale: image %dx%d outside 1..8192", w, h);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 31) == 0, "sst_rescale: rows must be 32-byte aligned (rows of 8 int32)");
  const int TH = rows_for(B, h, w);
  const int ntx = (w + COLS - 1) / COLS;
  const int64_t ntile = (int64_t)ntx * ((h + TH - 1) / TH);
  SST_REQUIRE(ntile <= 0x7fffffff, "sst_rescale: %lld tiles per plane", (long long)ntile);
  const int64_t lds = lds_bytes(TH);
  SST_REQUIRE(lds <= deg::LDS_BUDGET, "sst_rescale: %lld B of LDS needed > 64 KiB", (long long)lds);
  rescale_kernel<<<dim3((unsigned)ntile, 3, B), deg::NT, (size_t)lds, sst_stream(stream)>>>(x, y, rows, h, w, quantise, TH, ntx);
  SST_LAUNCH_CHECK("rescale_kernel");
  return SST_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sst_rescale_to: the random resize of the FIRST degradation stage.  sst_rescale's chain with an output
// geometry of its own: x [B,3,H,W] -> (hi, wi) with m1, the noise there, -> y [B,3,h,w] with m2, clamp and the 1/255 grid; the
// rows, the one-axis rule, the noise and the fmaf chains are the ones above (the device functions are shared).  Two things differ.
// The ratios: 8 hi >= H and hi <= 2 H, while h <= H <= 16 h, so an area tap count is no longer bounded by TAPS (H -> hi: up to 9,
// hi -> h: up to 2 H / h + 1) - area weights are uniform, so an entry keeps its first tap, its count and ONE weight, and only the
// bilinear / bicubic entries keep a weight per tap.  And the tile: an output pixel names up to 2 H / h intermediate rows, so the
// launcher takes the output tile from the launch's H / h and W / w (at x4: 8 x 8 outputs over an intermediate rectangle of at most
// 69 x 69), the largest whose LDS stays under TILE_LDS; SST_RESIZE1_TILE=RxC (dev switch) fixes it.  No pixel depends on it.
namespace {

constexpr int WTAPS = 4;                        // weights kept per entry: bicubic 4, bilinear 2, area one
constexpr int RATIO_TO = 2, MIN_DIV_TO = 8;     // hi <= 2 H, 8 hi >= H
constexpr int MAX_DOWN_TO = 16;                 // H <= 16 h
constexpr int64_t TILE_LDS = 28 * 1024;         // the launcher halves the tile until its LDS is below this (5 workgroups per CU)

// the intermediate rows that T output rows can name: T (2 N / n) rounded up, plus the widest mode's reach at both ends
__host__ __device__ constexpr int nin_for(int T, int N, int n) { return (int)((2ll * N * T + n - 1) / n) + 5; }

struct TableTo {
  int* base;
  int* n;
  float* w;
  int L;
  __device__ TableTo(float* p, int L_) : base(reinterpret_cast<int*>(p)), n(reinterpret_cast<int*>(p) + L_), w(p + 2 * L_), L(L_) {}
  __host__ __device__ static constexpr int floats(int L_) { return (2 + WTAPS) * L_; }
};

__device__ __forceinline__ void make_taps_to(const TableTo& T, int slot, int mode, int i, int n_in, int n_out) {
  const int L = T.L;
  if (mode == 0) {                               // the count as it is: no cap
    const int a = (i * n_in) / n_out, b = ((i + 1) * n_in + n_out - 1) / n_out;
    T.base[slot] = a, T.n[slot] = b - a, T.w[slot] = 1.f / (float)(b - a);
    return;
  }
  Frac q = frac(i, n_in, n_out);
  if (mode == 1) {
    if (q.f < 0) q.f = 0, q.t = 0.f;
    T.base[slot] = q.f, T.n[slot] = 2;
    T.w[slot] = 1.f - q.t, T.w[L + slot] = q.t;
  } else {
    T.base[slot] = q.f - 1, T.n[slot] = 4;
    T.w[slot] = cc2(q.t + 1.f), T.w[L + slot] = cc1(q.t), T.w[2 * L + slot] = cc1(1.f - q.t), T.w[3 * L + slot] = cc2(2.f - q.t);
  }
}

__global__ __launch_bounds__(deg::NT) void rescale_to_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             const int* __restrict__ rows, int H, int W, int h, int w, int quantise,
                                                             int TH, int TW, int ntx, int NIY, int NIX) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const int r0 = ty * TH, nr = min(TH, h - r0), c0 = tx * TW, nc = min(TW, w - c0);
  const float* __restrict__ img = x + ((int64_t)b * 3 + c) * H * W;
  float* __restrict__ out = y + ((int64_t)b * 3 + c) * h * w;
  const Row q = load_row(rows, b);
  const bool same = H == h && W == w;

  // ---- the workgroup-uniform exits
  const bool sized = q.hi != 0 || q.wi != 0;
  const bool bad = q.hi < 0 || q.wi < 0 || (q.hi == 0) != (q.wi == 0) || q.m1 == 3 || q.m2 == 3 || q.high != 0 || !(q.sn >= 0.f) ||
                   !(q.sp >= 0.f) ||
                   (sized && ((int64_t)MIN_DIV_TO * q.hi < H || q.hi > RATIO_TO * H || (int64_t)MIN_DIV_TO * q.wi < W || q.wi > RATIO_TO * W));
  if (bad) {
    for (int i = tid; i < nr * nc; i += deg::NT) out[(int64_t)(r0 + i / nc) * w + c0 + i % nc] = __builtin_nanf("");
    return;
  }
  const bool noisy = q.sn != 0.f || q.sp != 0.f;
  if (same && !sized && !noisy) {                                // sst_rescale's pass-through: the bits (equal geometry only)
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(img);
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out);
    for (int i = tid; i < nr * nc; i += deg::NT) {
      const int64_t o = (int64_t)(r0 + i / nc) * w + c0 + i % nc;
      dst[o] = src[o];
    }
    return;
  }
  if (same && !sized) {                                          // sst_rescale's noise at the image's own size
    const uint32_t e0 = q.gray ? 0u : (uint32_t)c * (uint32_t)(h * w);
    for (int i = tid; i < nr * nc; i += deg::NT) {
      const int rr = i / nc, yy = r0 + rr, xx = c0 + (i - rr * nc);
      float v = img[(int64_t)yy * w + xx];
      const float z = deg::gauss(e0 + (uint32_t)(yy * w + xx), q.k0, q.k1);
      const float sd = q.sp == 0.f ? q.sn : sqrtf(fmaf(q.sp, fmaxf(v, 0.f), q.sn * q.sn));
      v = fmaf(sd, z, v);
      out[(int64_t)yy * w + xx] = finish(v, quantise);
    }
    return;
  }

  // ---- the intermediate pixels that this tile's second resize names: rows [Y0, Y1], columns [X0, X1].  "keep": the input itself
  const int hi = sized ? q.hi : H, wi = sized ? q.wi : W;
  int Y0, Y1, X0, X1, unused;
  tap_span(q.m2, r0, hi, h, Y0, unused);
  tap_span(q.m2, r0 + nr - 1, hi, h, unused, Y1);
  tap_span(q.m2, c0, wi, w, X0, unused);
  tap_span(q.m2, c0 + nc - 1, wi, w, unused, X1);
  const int nyi = Y1 - Y0 + 1, nxi = X1 - X0 + 1, PITCH_TO = NIX | 1;
  if (nyi < 1 || nxi < 1 || nyi > NIY || nxi > NIX) {            // cannot be within the limits above: no write outside LDS
    for (int i = tid; i < nr * nc; i += deg::NT) out[(int64_t)(r0 + i / nc) * w + c0 + i % nc] = __builtin_nanf("");
    return;
  }

  float* s_u = lds;                                              // [NIY][PITCH_TO]
  const TableTo t_iy(s_u + NIY * PITCH_TO, NIY), t_ix(t_iy.w + WTAPS * NIY, NIX), t_oy(t_ix.w + WTAPS * NIX, TH),
      t_ox(t_oy.w + WTAPS * TH, TW);
  const int first = sized ? 0 : nyi + nxi;                       // keep: no first resize, no tables for it
  for (int i = first + tid; i < nyi + nxi + nr + nc; i += deg::NT) {
    if (i < nyi) make_taps_to(t_iy, i, q.m1, Y0 + i, H, hi);
    else if (i < nyi + nxi) make_taps_to(t_ix, i - nyi, q.m1, X0 + i - nyi, W, wi);
    else if (i < nyi + nxi + nr) make_taps_to(t_oy, i - nyi - nxi, q.m2, r0 + i - nyi - nxi, hi, h);
    else make_taps_to(t_ox, i - nyi - nxi - nr, q.m2, c0 + i - nyi - nxi - nr, wi, w);
  }
  __syncthreads();

  // ---- phase 1: u[Y][X] = sum_j wy[j] (sum_i wx[i] x[iy_j][ix_i]), then the noise at the intermediate resolution
  const uint32_t e0 = q.gray ? 0u : (uint32_t)c * (uint32_t)(hi * wi);
  const int sy1 = q.m1 == 0 ? 0 : NIY, sx1 = q.m1 == 0 ? 0 : NIX;  // an area entry has one weight for all its taps
  for (int i = tid; i < nyi * nxi; i += deg::NT) {
    const int ry = i / nxi, rx = i - ry * nxi;
    float v;
    if (sized) {
      const int by = t_iy.base[ry], ny = t_iy.n[ry], bx = t_ix.base[rx], nx = t_ix.n[rx];
      v = 0.f;
      for (int j = 0; j < ny; ++j) {
        const float* __restrict__ src = img + (int64_t)min(max(by + j, 0), H - 1) * W;
        float r = 0.f;
        for (int k = 0; k < nx; ++k) r = fmaf(t_ix.w[k * sx1 + rx], src[min(max(bx + k, 0), W - 1)], r);
        v = fmaf(t_iy.w[j * sy1 + ry], r, v);
      }
    } else {
      v = img[(int64_t)(Y0 + ry) * W + X0 + rx];
    }
    if (noisy) {
      const float z = deg::gauss(e0 + (uint32_t)((Y0 + ry) * wi + X0 + rx), q.k0, q.k1);
      const float sd = q.sp == 0.f ? q.sn : sqrtf(fmaf(q.sp, fmaxf(v, 0.f), q.sn * q.sn));
      v = fmaf(sd, z, v);
    }
    s_u[ry * PITCH_TO + rx] = v;
  }
  __syncthreads();

  // ---- phase 2: to (h, w) by the same rule on u, clamp, quantise
  const int sy2 = q.m2 == 0 ? 0 : TH, sx2 = q.m2 == 0 ? 0 : TW;
  for (int i = tid; i < nr * nc; i += deg::NT) {
    const int rr = i / nc, cc = i - rr * nc;
    const int by = t_oy.base[rr], ny = t_oy.n[rr], bx = t_ox.base[cc], nx = t_ox.n[cc];
    float v = 0.f;
    for (int j = 0; j < ny; ++j) {
      const float* src = s_u + (min(max(by + j, Y0), Y1) - Y0) * PITCH_TO;     // (a tap is inside the rectangle: the clamp is the
      float r = 0.f;                                                            // model's at the image's edge, and holds LDS reads in)
      for (int k = 0; k < nx; ++k) r = fmaf(t_ox.w[k * sx2 + cc], src[min(max(bx + k, X0), X1) - X0], r);
      v = fmaf(t_oy.w[j * sy2 + rr], r, v);
    }
    out[(int64_t)(r0 + rr) * w + c0 + cc] = finish(v, quantise);
  }
}

struct TileTo {
  int TH, TW, NIY, NIX;
  int64_t lds;
};

TileTo tile_to(int TH, int TW, int H, int W, int h, int w) {
  const int NIY = nin_for(TH, H, h), NIX = nin_for(TW, W, w);
  return {TH, TW, NIY, NIX,
          4 * ((int64_t)NIY * (NIX | 1) + TableTo::floats(NIY) + TableTo::floats(NIX) + TableTo::floats(TH) + TableTo::floats(TW))};
}

// The output tile: ROWS x COLS, the side with the longer intermediate extent halved until the LDS is below TILE_LDS (1 x 1 at
// the least).  SST_RESIZE1_TILE=RxC (dev switch; R, C in 1..32) fixes it.  A pixel's value does not depend on it.
TileTo tile_for(int H, int W, int h, int w) {
  if (const char* e = sst_env("SST_RESIZE1_TILE")) {
    char* end = nullptr;
    const long r = strtol(e, &end, 10);
    const long c = end && (*end == 'x' || *end == 'X') ? strtol(end + 1, nullptr, 10) : 0;
    if (r >= 1 && r <= ROWS && c >= 1 && c <= COLS) return tile_to((int)r, (int)c, H, W, h, w);
  }
  TileTo t = tile_to(ROWS, COLS, H, W, h, w);
  while (t.lds > TILE_LDS && (t.TH > 1 || t.TW > 1))
    t = (t.TW == 1 || (t.TH > 1 && t.NIY >= t.NIX)) ? tile_to(t.TH >> 1, t.TW, H, W, h, w) : tile_to(t.TH, t.TW >> 1, H, W, h, w);
  return t;
}

}  // namespace

SST_API int sst_rescale_to(const float* x, float* y, const int* rows, int B, int H, int W, int h, int w, int quantise, void* stream) {
  SST_REQUIRE(x && y && rows, "sst_rescale_to: null pointer");
  SST_REQUIRE(x != y, "sst_rescale_to: y == x (a tile reads its neighbours' pixels: out of place only)");
  SST_REQUIRE(B > 0 && B <= 65535, "sst_rescale_to: batch %d outside [1, 65535]", B);
  SST_REQUIRE(H > 0 && W > 0 && H <= 8192 && W <= 8192, "sst_rescale_to: input image %dx%d outside 1..8192", W, H);
  SST_REQUIRE(h > 0 && w > 0 && h <= 8192 && w <= 8192, "sst_rescale_to: output image %dx%d outside 1..8192", w, h);
  SST_REQUIRE(h <= H && w <= W, "sst_rescale_to: the output %dx%d is larger than the input %dx%d", w, h, W, H);
  SST_REQUIRE(H <= MAX_DOWN_TO * h && W <= MAX_DOWN_TO * w, "sst_rescale_to: the input %dx%d is more than %d times the output %dx%d", W,
              H, MAX_DOWN_TO, w, h);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 31) == 0, "sst_rescale_to: rows must be 32-byte aligned (rows of 8 int32)");
  const TileTo t = tile_for(H, W, h, w);
  const int ntx = (w + t.TW - 1) / t.TW;
  const int64_t ntile = (int64_t)ntx * ((h + t.TH - 1) / t.TH);
  SST_REQUIRE(ntile <= 0x7fffffff, "sst_rescale_to: %lld tiles per plane", (long long)ntile);
  SST_REQUIRE(t.lds <= deg::LDS_BUDGET, "sst_rescale_to: %lld B of LDS needed by a %dx%d tile (%dx%d -> %dx%d) > 64 KiB", (long long)t.lds,
              t.TH, t.TW, W, H, w, h);
  rescale_to_kernel<<<dim3((unsigned)ntile, 3, B), deg::NT, (size_t)t.lds, sst_stream(stream)>>>(x, y, rows, H, W, h, w, quantise, t.TH,
                                                                                                t.TW, ntx, t.NIY, t.NIX);
  SST_LAUNCH_CHECK("rescale_to_kernel");
  return SST_OK;
}
