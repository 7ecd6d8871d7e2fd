// sst_degrade: the degradation stage of degrade.h on an fp32 batch x [B,3,H,W] of any size - the stand-alone form of what
// sst_gather_crops_degraded (data.hip) does to its own gt, through the same device functions, so the two agree bit for bit.
//
// One workgroup per (sample, channel, band of R <= deg::ROWS_MAX LR rows, tile of deg::TILE_COLS LR columns): a 1024-px row band
// does not fit the LDS, a column tile of 16 LR pixels (x4: 76 blur columns, a plane row of 101 floats at K = 21) does.  The workgroup
// reads its plane straight from x with torch's `reflect` map at the IMAGE border; R is the largest band height whose LDS fits 64 KiB.
#include "degrade.h"
#include <algorithm>

namespace {

__global__ __launch_bounds__(deg::NT) void degrade_kernel(
    const float* __restrict__ x, const int* __restrict__ dg, int H, int W, int K, int quantise, float* __restrict__ lr,
    const float* __restrict__ wy, const int* __restrict__ iy, const float* __restrict__ wx, const int* __restrict__ ix, int oh, int ow,
    int Ty, int Tx, int R, int nct, int nr_max, int nc_max) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int ct = blockIdx.x % nct, band = blockIdx.x / nct;
  const deg::Layout L(K, R, nr_max, nc_max, 0, 0);
  const int p = L.p;
  deg::Tile t;
  t.oy0 = band * R, t.noy = min(R, oh - t.oy0), t.ox0 = ct * deg::TILE_COLS, t.nox = min(deg::TILE_COLS, ow - t.ox0);
  float* lr_plane = lr + ((int64_t)b * 3 + c) * oh * ow;

  // ---- the tile: rows from all of the band's taps; columns from the first and the last LR column's (the tables are monotone; an
  // entry that is not is clamped into the tile by the passes)
  int r1, c1 = -1;
  bool ok = deg::tap_rows(iy, Ty, t.oy0, t.noy, H, t.r0, r1);
  t.c0 = W;
  for (int tx = 0; tx < Tx; ++tx) {
    t.c0 = min(t.c0, ix[(int64_t)t.ox0 * Tx + tx]);
    c1 = max(c1, ix[(int64_t)(t.ox0 + t.nox - 1) * Tx + tx]);
  }
  t.nr = r1 - t.r0 + 1, t.nc = c1 - t.c0 + 1;
  ok = ok && t.c0 >= 0 && c1 < W && t.nc >= 1 && t.nr <= nr_max && t.nc <= nc_max;
  if (!ok) return deg::fill_nan(lr_plane, t, ow);

  const deg::Params q = deg::load_params(dg, b);
  float* s_k = reinterpret_cast<float*>(smem + L.o_k);
  if (q.blur()) {
    deg::weights_raw(s_k, q, K);
    __syncthreads();
    if (tid == deg::NT - 1) deg::weights_sum(s_k, reinterpret_cast<double*>(smem), K);
  }
  // ---- the plane, reflected at the image border (p < min(H, W): one reflection lands inside)
  float* plane = reinterpret_cast<float*>(smem + L.o_plane);
  const float* img = x + ((int64_t)b * 3 + c) * H * W;
  const int wp = t.nc + 2 * p;
  for (int i = tid; i < (t.nr + 2 * p) * wp; i += deg::NT) {
    const int r = i / wp, j = i - r * wp;
    plane[r * L.pitch + j] = img[(int64_t)deg::refl(t.r0 - p + r, H) * W + deg::refl(t.c0 - p + j, W)];
  }
  __syncthreads();
  deg::finish_tile(smem, L, t, q, K, quantise, lr_plane, (uint32_t)c * (uint32_t)(oh * ow), wy, iy, wx, ix, ow, Ty, Tx);
}

}  // namespace

SST_API int sst_degrade_tile_cols(void) { return deg::TILE_COLS; }

SST_API int sst_degrade(const float* x, const int* dg, int B, int H, int W, int K, int quantise, float* lr, const float* wy,
                        const int* iy, const float* wx, const int* ix, int oh, int ow, int Ty, int Tx, void* stream) {
  SST_REQUIRE(x && dg && lr && wy && iy && wx && ix, "sst_degrade: null pointer");
  SST_REQUIRE(B > 0 && B <= 65535, "sst_degrade: batch %d outside [1, 65535]", B);
  SST_REQUIRE(K >= deg::K_MIN && K <= deg::K_MAX && (K & 1), "sst_degrade: the blur window K = %d must be odd and in %d..%d", K,
              deg::K_MIN, deg::K_MAX);
  SST_REQUIRE(H > 0 && W > 0 && H <= 32768 && W <= 32768, "sst_degrade: image %dx%d outside 1..32768", W, H);
  SST_REQUIRE(K / 2 < (H < W ? H : W), "sst_degrade: the half window %d (K = %d) must be smaller than the image's shorter side (%dx%d)",
              K / 2, K, W, H);
  SST_REQUIRE(oh > 0 && ow > 0 && oh <= H && ow <= W && Ty > 0 && Tx > 0 && Ty <= 64 && Tx <= 64,
              "sst_degrade: bad LR arguments (%dx%d -> %dx%d, %d / %d taps)", W, H, ow, oh, Ty, Tx);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(dg) & 31) == 0, "sst_degrade: deg must be 32-byte aligned (rows of 8 int32)");
  // taps of consecutive LR pixels move by the scale, which is at most H / oh (W / ow): the bound of a band's (tile's) extent
  const int tw = ow < deg::TILE_COLS ? ow : deg::TILE_COLS;
  const int nc_max = (int)std::min<int64_t>(W, Tx + (int64_t)(tw - 1) * (W / ow));
  int R = oh < deg::ROWS_MAX ? oh : deg::ROWS_MAX, nr_max = 0;
  int64_t lds = 0;
  for (; R >= 1; --R) {
    nr_max = (int)std::min<int64_t>(H, Ty + (int64_t)(R - 1) * (H / oh));
    lds = deg::Layout(K, R, nr_max, nc_max, 0, 0).bytes;
    if (lds <= deg::LDS_BUDGET) break;
  }
  SST_REQUIRE(R >= 1, "sst_degrade: %lld B of LDS needed (K %d, %d / %d taps, scale about %d) > 64 KiB", (long long)lds, K, Ty, Tx,
              W / ow);
  const int nct = (ow + deg::TILE_COLS - 1) / deg::TILE_COLS;
  const int64_t ntile = (int64_t)nct * ((oh + R - 1) / R);
  SST_REQUIRE(ntile <= 0x7fffffff, "sst_degrade: %lld tiles per plane", (long long)ntile);
  degrade_kernel<<<dim3((unsigned)ntile, 3, B), deg::NT, (size_t)lds, sst_stream(stream)>>>(x, dg, H, W, K, quantise, lr, wy, iy, wx, ix,
                                                                                           oh, ow, Ty, Tx, R, nct, nr_max, nc_max);
  SST_LAUNCH_CHECK("degrade_kernel");
  return SST_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// sst_blur: step (1) of degrade.h alone, at the input's size: y = x (*) k per sample, unquantised, through the
// device functions above - the weights, the fp64 sum, `reflect` at the image border and blur_tile's row-major fmaf chain - so a
// sample's blurred image is the one degrade_kernel makes in LDS before its bicubic.  A row with qa < 0 keeps the sample's bits.  One
// workgroup per (sample, channel, tile of BLUR_ROWS x BLUR_COLS pixels): 256 threads x 4 adjacent pixels, blur_tile's own shape.
namespace {

constexpr int BLUR_ROWS = 32, BLUR_COLS = 32;

__global__ __launch_bounds__(deg::NT) void blur_kernel(const float* __restrict__ x, const int* __restrict__ dg, float* __restrict__ y,
                                                       int H, int W, int K, int nct) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const int r0 = (blockIdx.x / nct) * BLUR_ROWS, c0 = (blockIdx.x % nct) * BLUR_COLS;
  const int nr = min(BLUR_ROWS, H - r0), nc = min(BLUR_COLS, W - c0);
  const float* __restrict__ img = x + ((int64_t)b * 3 + c) * H * W;
  float* __restrict__ out = y + ((int64_t)b * 3 + c) * H * W;
  const deg::Params q = deg::load_params(dg, b);
  if (!q.blur()) {                                               // the bits, whatever they are
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(img);
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out);
    for (int i = tid; i < nr * nc; i += deg::NT) {
      const int64_t o = (int64_t)(r0 + i / nc) * W + c0 + i % nc;
      dst[o] = src[o];
    }
    return;
  }
  const deg::Layout L(K, 0, BLUR_ROWS, BLUR_COLS, 0, 0);
  const int p = L.p;
  float* s_k = reinterpret_cast<float*>(smem + L.o_k);
  deg::weights_raw(s_k, q, K);
  __syncthreads();
  if (tid == deg::NT - 1) deg::weights_sum(s_k, reinterpret_cast<double*>(smem), K);
  float* plane = reinterpret_cast<float*>(smem + L.o_plane);     // reflected at the image border (p < min(H, W))
  const int wp = nc + 2 * p;
  for (int i = tid; i < (nr + 2 * p) * wp; i += deg::NT) {
    const int r = i / wp, j = i - r * wp;
    plane[r * L.pitch + j] = img[(int64_t)deg::refl(r0 - p + r, H) * W + deg::refl(c0 - p + j, W)];
  }
  __syncthreads();
  deg::weights_norm(s_k, reinterpret_cast<const double*>(smem), K);
  __syncthreads();
  float* s_blur = reinterpret_cast<float*>(smem + L.o_a);
  deg::blur_tile(plane, L.pitch, s_k, K, s_blur, L.bpitch, nr, nc);
  __syncthreads();
  for (int i = tid; i < nr * nc; i += deg::NT) {
    const int r = i / nc, j = i - r * nc;
    out[(int64_t)(r0 + r) * W + c0 + j] = s_blur[r * L.bpitch + j];
  }
}

}  // namespace

SST_API int sst_blur(const float* x, const int* dg, float* y, int B, int H, int W, int K, void* stream) {
  SST_REQUIRE(x && dg && y, "sst_blur: null pointer");
  SST_REQUIRE(x != y, "sst_blur: y == x (a tile reads its neighbours' pixels: out of place only)");
  SST_REQUIRE(B > 0 && B <= 65535, "sst_blur: batch %d outside [1, 65535]", B);
  SST_REQUIRE(K >= deg::K_MIN && K <= deg::K_MAX && (K & 1), "sst_blur: the blur window K = %d must be odd and in %d..%d", K, deg::K_MIN,
              deg::K_MAX);
  SST_REQUIRE(H > 0 && W > 0 && H <= 32768 && W <= 32768, "sst_blur: image %dx%d outside 1..32768", W, H);
  SST_REQUIRE(K / 2 < (H < W ? H : W), "sst_blur: the half window %d (K = %d) must be smaller than the image's shorter side (%dx%d)",
              K / 2, K, W, H);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(dg) & 31) == 0, "sst_blur: deg must be 32-byte aligned (rows of 8 int32)");
  const int nct = (W + BLUR_COLS - 1) / BLUR_COLS;
  const int64_t ntile = (int64_t)nct * ((H + BLUR_ROWS - 1) / BLUR_ROWS);
  const int64_t lds = deg::Layout(K, 0, BLUR_ROWS, BLUR_COLS, 0, 0).bytes;
  SST_REQUIRE(lds <= deg::LDS_BUDGET, "sst_blur: %lld B of LDS needed > 64 KiB", (long long)lds);
  blur_kernel<<<dim3((unsigned)ntile, 3, B), deg::NT, (size_t)lds, sst_stream(stream)>>>(x, dg, y, H, W, K, nct);
  SST_LAUNCH_CHECK("blur_kernel");
  return SST_OK;
}
