// Back-projection loss (loss.py: BackProjectionLoss; metrics.py: lr_consistency), forward and backward, for gfx950: the
// super-resolved image, downscaled by the antialiased bicubic kernel that made the LR input, compared with that LR input.
//
//   down(x)[oy][ox] = sum_tx wx[ox][tx] * V[oy][ix[ox][tx]],   V[oy][c] = sum_ty wy[oy][ty] * x[iy[oy][ty]][c]
//     - bicubic_kernel's arithmetic (misc.hip): fp32 FMAs, taps in table order, the vertical sum inside; host-built tap tables
//       (bicubic.py: weights normalised, border indices clamped), 1/scale with scale 2, 4 or 8, oh = H / scale, ow = W / scale
//   T = rintf(255 down(gt)) / 255 (the bits of sst_bicubic(gt, round_grid = 1)), the unrounded down(gt), or a given LR image
//   D = down(sr) - T,  loss = mean over B*3*oh*ow of |D| (criterion 0, "l1") or D^2 (criterion 1, "mse")
//
// Forward: one workgroup per (image plane, band of 8 LR rows, tile of 32 LR columns - 16 at x8).  The tile's input columns are one
// contiguous span [c_lo, c_hi] of at most 160 (the taps of neighbouring outputs overlap); the workgroup forms the vertical sums of sr
// (and of gt) over that span with coalesced row reads - thread = (LR row, input column), walking the input rows of its Ty taps -
// into LDS, 2 x 8 x 160 floats whatever the image size, then one thread per LR pixel finishes the horizontal sum from LDS, forms D and,
// with saved != null, stores rho'(D) (sign(D), sign(0) = 0, or 2 D) to the saved map [B,3,oh,ow].  rho(D) is reduced in fp64: one
// partial per workgroup, the last-arriving workgroup sums them in index order (and per image, for per_image) and re-arms the
// counter: no floating-point atomics, the same bits in every run and replay.
//
// Backward: a gather through the transposed tap tables, one thread per HR pixel.  Row r lists the (LR row, weight) pairs whose
// taps read it - ti_y [H][Ny] / tw_y; column c likewise, ti_x [W][Nx] / tw_x - the taps of one output that were clamped onto a
// border pixel merged into one entry by the host, so no list is longer than an interior one; the lists are packed to the front
// and end at the first index < 0 (pads are skipped, not multiplied by zero, so a NaN of the map reaches exactly the pixels under
// its taps):
//   dsr[r][c] (+)= scale * sum_(ox,b) in column list  b * sum_(oy,a) in row list  a * saved[oy][ox]
//
// This file spells every FMA out; nothing depends on the contraction mode.
#include "common.h"

#include <cmath>

namespace {

constexpr int BP_NT = 256;
constexpr int BP_ROWS = 8;             // LR rows per band
constexpr int BP_SPAN = 160;           // input columns a tile may span: (tile - 1) * scale + taps <= 160 at every built scale
constexpr int BP_MAX_LIST = 64;        // the longest transposed list the backward walks

__host__ __device__ constexpr int bp_tile(int scale) { return scale == 8 ? 16 : 32; }      // LR columns per tile

__global__ __launch_bounds__(BP_NT) void bp_loss_fwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                            const float* __restrict__ lr, float* __restrict__ saved,
                                                            double* partials, unsigned* counter, float* __restrict__ loss,
                                                            double* __restrict__ per_image, const float* __restrict__ wy,
                                                            const int* __restrict__ iy, const float* __restrict__ wx,
                                                            const int* __restrict__ ix, int H, int W, int oh, int ow, int Ty, int Tx,
                                                            int tile, int criterion, int round_target, int clamp_sr, double count) {
  __shared__ float s_v[2][BP_ROWS][BP_SPAN];
  __shared__ double s_red[BP_NT / 64];
  __shared__ unsigned s_flag;
  const int tid = threadIdx.x, z = blockIdx.z;
  const int ox0 = blockIdx.x * tile, oy0 = blockIdx.y * BP_ROWS;
  const int ncol = min(tile, ow - ox0), nrow = min(BP_ROWS, oh - oy0);
  // the tile's input columns: the indices grow with the output and with the tap, so the first and the last entry bound them
  const int c_lo = min(max(ix[(int64_t)ox0 * Tx], 0), W - 1);
  const int c_hi = min(max(ix[(int64_t)(ox0 + ncol - 1) * Tx + Tx - 1], c_lo), W - 1);
  const int span = min(c_hi - c_lo + 1, BP_SPAN);
  const int64_t hw = (int64_t)H * W, ohw = (int64_t)oh * ow;
  const float* xs = sr + (int64_t)z * hw + c_lo;
  const float* xg = gt ? gt + (int64_t)z * hw + c_lo : nullptr;

  // ---- vertical sums over the span: thread = (LR row, input column); a wave reads 64 consecutive floats of each tap's row
  for (int i = tid; i < nrow * span; i += BP_NT) {
    const int r = i / span, c = i - r * span;
    const float* pw = wy + (int64_t)(oy0 + r) * Ty;
    const int* pi = iy + (int64_t)(oy0 + r) * Ty;
    float vs = 0.f, vg = 0.f;
    for (int t = 0; t < Ty; ++t) {
      const int64_t o = (int64_t)min(max(pi[t], 0), H - 1) * W + c;
      const float w = pw[t];
      float x = xs[o];
      if (clamp_sr) x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);          // a NaN stays a NaN
      vs = fmaf(x, w, vs);
      if (xg) vg = fmaf(xg[o], w, vg);
    }
    s_v[0][r][c] = vs;
    s_v[1][r][c] = vg;
  }
  __syncthreads();

  // ---- horizontal sums, D, rho'(D) and rho(D): one thread per LR pixel of the tile
  double ss = 0.0;
  for (int i = tid; i < nrow * ncol; i += BP_NT) {
    const int r = i / ncol, o = i - r * ncol;
    const int oy = oy0 + r, ox = ox0 + o;
    const float* pw = wx + (int64_t)ox * Tx;
    const int* pi = ix + (int64_t)ox * Tx;
    float as = 0.f, ag = 0.f;
    for (int t = 0; t < Tx; ++t) {
      const int c = min(max(pi[t] - c_lo, 0), span - 1);
      const float w = pw[t];
      as = fmaf(s_v[0][r][c], w, as);
      ag = fmaf(s_v[1][r][c], w, ag);
    }
    const int64_t q = (int64_t)z * ohw + (int64_t)oy * ow + ox;
    float T;
    if (lr)
      T = lr[q];
    else
      T = round_target ? rintf(255.f * ag) / 255.f : ag;
    const float D = as - T;
    const double d = (double)D;
    ss += criterion == 0 ? fabs(d) : d * d;
    if (saved) saved[q] = criterion == 0 ? (D > 0.f ? 1.f : (D < 0.f ? -1.f : D)) : 2.f * D;      // sign(0) = 0, sign(NaN) = NaN
  }

  // ---- one partial per workgroup; the last arriver sums them in index order and re-arms the counter
  const unsigned per_plane = gridDim.x * gridDim.y, nblk = per_plane * gridDim.z;
  const unsigned blk = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  if (!last_block_arrive_d<BP_NT>(ss, partials, blk, counter, nblk, &s_flag, s_red)) return;
  if (per_image) {                                   // image b owns the 3 * per_plane consecutive partials of its planes
    const unsigned per_img = 3 * per_plane, nimg = gridDim.z / 3;
    for (unsigned b = tid; b < nimg; b += BP_NT) {
      double t = 0.0;
      for (unsigned k = 0; k < per_img; ++k) t += load_agent_d(partials + (int64_t)b * per_img + k);
      per_image[b] = t / (3.0 * (double)oh * (double)ow);
    }
  }
  const double t = last_block_total_d<BP_NT>(partials, counter, nblk, s_red);
  if (tid == 0) loss[0] = (float)(t / count);
}

// dsr (+)= scale * (scale_dev ? *scale_dev : 1) * down^T(saved);  scale = scale_host / count.  Block = 64 columns x 4 rows.
__global__ __launch_bounds__(BP_NT) void bp_loss_bwd_kernel(const float* __restrict__ saved, float* __restrict__ dsr,
                                                            const float* __restrict__ tw_y, const int* __restrict__ ti_y,
                                                            const float* __restrict__ tw_x, const int* __restrict__ ti_x,
                                                            const float* __restrict__ scale_dev, double scale, int accumulate, int H,
                                                            int W, int oh, int ow, int Ny, int Nx) {
  // a wave is 64 columns of one row: the row list is wave-uniform (scalar loads), the column list is read once per entry
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= W || r >= H) return;
  const int z = blockIdx.z;
  const float* m = saved + (int64_t)z * oh * ow;
  const float* pwy = tw_y + (int64_t)r * Ny;
  const int* piy = ti_y + (int64_t)r * Ny;
  const float* pwx = tw_x + (int64_t)c * Nx;
  const int* pix = ti_x + (int64_t)c * Nx;
  float acc = 0.f;
  for (int b = 0; b < Nx; ++b) {
    const int ox = pix[b];
    if (ox < 0 || ox >= ow) break;                    // the end of the list (or a table that is not this shape's: nothing is read)
    const float wb = pwx[b];
    float v = 0.f;
    for (int a = 0; a < Ny; ++a) {
      const int oy = piy[a];
      if (oy < 0 || oy >= oh) break;
      v = fmaf(m[(int64_t)oy * ow + ox], pwy[a], v);
    }
    acc = fmaf(v, wb, acc);
  }
  double sc = scale;
  if (scale_dev) sc = sc * (double)scale_dev[0];
  const float vf = (float)((double)acc * sc);
  const int64_t o = (int64_t)z * H * W + (int64_t)r * W + c;
  dsr[o] = accumulate ? dsr[o] + vf : vf;
}

// shape rules shared by the three entries
static int bp_check_shape(const char* who, int B, int H, int W, int scale) {
  SST_REQUIRE(scale == 2 || scale == 4 || scale == 8, "%s: scale must be 2, 4 or 8, got %d", who, scale);
  SST_REQUIRE(B > 0 && (int64_t)B * 3 <= 65535, "%s: bad batch %d (1 <= B <= 21845)", who, B);
  SST_REQUIRE(H >= scale && W >= scale, "%s: image %dx%d is below the %d-px minimum of scale %d", who, W, H, scale, scale);
  SST_REQUIRE((H + 3) / 4 <= 65535, "%s: image height %d needs more than 65535 row blocks", who, H);
  return SST_OK;
}

static int64_t bp_bands(int H, int scale) { return (H / scale + BP_ROWS - 1) / BP_ROWS; }
static int64_t bp_tiles(int W, int scale) { return (W / scale + bp_tile(scale) - 1) / bp_tile(scale); }

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_bp_loss_workspace(int B, int H, int W, int scale, int64_t* saved_floats, int64_t* partial_floats) {
  SST_REQUIRE(saved_floats && partial_floats, "sst_bp_loss_workspace: null pointer");
  if (int rc = bp_check_shape("sst_bp_loss_workspace", B, H, W, scale)) return rc;
  *saved_floats = (int64_t)B * 3 * (H / scale) * (int64_t)(W / scale);
  *partial_floats = 2 * (int64_t)B * 3 * bp_bands(H, scale) * bp_tiles(W, scale);          // one fp64 partial per workgroup
  return SST_OK;
}

SST_API int sst_bp_loss_fwd(const float* sr, const float* gt, const float* lr, float* loss, double* per_image, float* saved,
                            float* partials, unsigned* counter, const float* wy, const int* iy, const float* wx, const int* ix, int B,
                            int H, int W, int scale, int Ty, int Tx, int criterion, int round_target, int clamp_sr, void* stream) {
  SST_REQUIRE(sr && loss && partials && counter && wy && iy && wx && ix, "sst_bp_loss_fwd: null pointer");
  SST_REQUIRE((gt != nullptr) != (lr != nullptr), "sst_bp_loss_fwd: exactly one of gt and lr must be given, got %s",
              gt ? "both" : "neither");
  SST_REQUIRE(!(saved && clamp_sr), "sst_bp_loss_fwd: clamp_sr is for the metric only - no saved map (no gradient) with it");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, "sst_bp_loss_fwd: partials must be 8-byte aligned");
  SST_REQUIRE(criterion == 0 || criterion == 1, "sst_bp_loss_fwd: criterion must be 0 (l1) or 1 (mse), got %d", criterion);
  if (int rc = bp_check_shape("sst_bp_loss_fwd", B, H, W, scale)) return rc;
  SST_REQUIRE(Ty >= 1 && Ty <= 4 * scale + 2 && Tx >= 1 && Tx <= 4 * scale + 2,
              "sst_bp_loss_fwd: %d / %d taps are not a scale-%d table (1 .. %d)", Ty, Tx, scale, 4 * scale + 2);
  static_assert((bp_tile(8) - 1) * 8 + 34 <= BP_SPAN && (bp_tile(4) - 1) * 4 + 18 <= BP_SPAN && (bp_tile(2) - 1) * 2 + 10 <= BP_SPAN,
                "a tile's input columns must fit the LDS span");
  const int oh = H / scale, ow = W / scale;
  SST_REQUIRE(bp_bands(H, scale) <= 65535, "sst_bp_loss_fwd: image height %d needs more than 65535 row bands", H);
  dim3 grid((unsigned)bp_tiles(W, scale), (unsigned)bp_bands(H, scale), B * 3);
  SST_REQUIRE((int64_t)grid.x * grid.y * grid.z < ((int64_t)1 << 31), "sst_bp_loss_fwd: too many tiles for %dx%d", W, H);
  const double count = (double)B * 3.0 * (double)oh * (double)ow;
  bp_loss_fwd_kernel<<<grid, BP_NT, 0, sst_stream(stream)>>>(sr, gt, lr, saved, reinterpret_cast<double*>(partials), counter, loss,
                                                             per_image, wy, iy, wx, ix, H, W, oh, ow, Ty, Tx, bp_tile(scale), criterion,
                                                             round_target, clamp_sr, count);
  SST_LAUNCH_CHECK("bp_loss_fwd_kernel");
  return SST_OK;
}

SST_API int sst_bp_loss_bwd(const float* saved, float* dsr, const float* tw_y, const int* ti_y, const float* tw_x, const int* ti_x,
                            const float* scale_dev, float scale_host, int accumulate, int B, int H, int W, int scale, int Ny, int Nx,
                            void* stream) {
  SST_REQUIRE(saved && dsr && tw_y && ti_y && tw_x && ti_x, "sst_bp_loss_bwd: null pointer");
  if (int rc = bp_check_shape("sst_bp_loss_bwd", B, H, W, scale)) return rc;
  SST_REQUIRE(Ny >= 1 && Ny <= BP_MAX_LIST && Nx >= 1 && Nx <= BP_MAX_LIST,
              "sst_bp_loss_bwd: transposed list widths %d / %d outside 1 .. %d", Ny, Nx, BP_MAX_LIST);
  const int oh = H / scale, ow = W / scale;
  dim3 grid((W + 63) / 64, (H + 3) / 4, B * 3);
  const double count = (double)B * 3.0 * (double)oh * (double)ow;
  bp_loss_bwd_kernel<<<grid, BP_NT, 0, sst_stream(stream)>>>(saved, dsr, tw_y, ti_y, tw_x, ti_x, scale_dev, (double)scale_host / count,
                                                             accumulate, H, W, oh, ow, Ny, Nx);
  SST_LAUNCH_CHECK("bp_loss_bwd_kernel");
  return SST_OK;
}
