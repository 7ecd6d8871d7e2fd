// Structure-tensor maps for gfx950: what the structure-tensor loss (st_loss.hip) integrates, as fields.  Analysis outputs, no
// gradient.
//
// Replaces (reference file:line)
//   structure_tensor                                utils.py:212-233   as used by visualization/ and data-exploration/
//   compute_invS1xS2 / compute_eigenvalues / compute_distance   utils.py:242-280   (the per-pixel distance before its mean)
//
// Layout: x, gt are NCHW fp32 [B,3,H,W].  Outputs, each optional (a null pointer = neither computed nor stored; the branch is
// uniform over the launch):
//   Sx, Sgt     [B,3,H,W]  (Jxx, Jyy, Jxy) of x / gt, the loss's plane order
//   Fx, Fgt     [B,3,H,W]  (t, c2, s2): t = Jxx + Jyy, c2 = (Jxx - Jyy) / (t + 1e-12), s2 = 2 Jxy / (t + 1e-12) - trace and the
//                          double-angle form of the orientation; orientation = atan2(s2, c2) / 2, coherence = hypot(c2, s2)
//   d           [B,H,W]    the distance st_pointwise() gives for (S(x), S(gt)): the loss's integrand
//   tile_sums   [B,tiles]  fp32 sum of d over the valid pixels of each 32x32 tile, tiles = ceil(H/32) * ceil(W/32), row-major
//
// Axis convention (st_tile.h): the reference's "x" is the HEIGHT axis.  An image that varies only from row to row has all its
// energy in Jxx (c2 = +1), one that varies only from column to column in Jyy (c2 = -1); sin(0.5 (col + row)) gives s2 = +1 and
// sin(0.5 (col - row)) gives s2 = -1.
//
// Same geometry and LDS budget as the loss forward: one workgroup of 1024 threads per 32x32 tile, the two images' tensors one after
// the other through the same LDS buffer.  Every workgroup writes only its own pixels and its own tile sum: no atomics, no counter,
// nothing to reset between calls; the per-image sum of the tile sums is the caller's (fp64, index order).
#include "st_tile.h"

namespace {

template <int R1, int R2>
__global__ __launch_bounds__(NT) void st_maps_kernel(const float* __restrict__ x, const float* __restrict__ gt, StMapsOut out, int H,
                                                     int W, int normalize, StTaps<R1, R2> tp) {
  __shared__ float lds[st_fwd_lds_floats<R1, R2>()];
  __shared__ float red[NT / 64];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W, img_off = (size_t)b * 3 * hw;
  const bool need1 = out.Sx || out.Fx || out.want_d(), need2 = out.Sgt || out.Fgt || out.want_d();
  float J1[PPT][3] = {}, J2[PPT][3] = {};
  if (need1) tile_structure_tensor<R1, R2>(x + img_off, H, W, y0, x0, tp, lds, J1);
  if (need2) tile_structure_tensor<R1, R2>(gt + img_off, H, W, y0, x0, tp, lds, J2);

  float lsum = 0.f;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int p = threadIdx.x + j * NT, y = y0 + (p >> 5), xx = x0 + (p & 31);
    if (y >= H || xx >= W) continue;                    // outside the image: neither stored nor summed
    maps_pixel(out, b, (size_t)y * W + xx, hw, J1[j], J2[j], normalize, lsum);
  }
  maps_tile_sum<NT>(out, b, lsum, red);
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_st_maps_workspace(int B, int H, int W, int64_t* tile_floats) {
  SST_REQUIRE(B > 0 && H > 0 && W > 0 && tile_floats, "sst_st_maps_workspace: bad shape");
  *tile_floats = tiles_of(B, H, W);
  return SST_OK;
}

SST_API int sst_st_maps(const float* x, const float* gt, float* Sx, float* Sgt, float* Fx, float* Fgt, float* d, float* tile_sums,
                        int B, int H, int W, float sigma, float rho, int normalize, void* stream) {
  SST_REQUIRE(x, "sst_st_maps: null pointer (x)");
  const StMapsOut out{Sx, Sgt, Fx, Fgt, d, tile_sums};
  if (const int rc = maps_args_ok("sst_st_maps", shape_ok(B, H, W, 65535), B, H, W, gt, out)) return rc;
  const int r1 = radius_of(sigma), r2 = radius_of(rho);
  const bool built = with_tile_build(r1, r2, [&](auto R1, auto R2) {
    st_maps_kernel<R1(), R2()><<<tiles_grid(H, W, B), NT, 0, sst_stream(stream)>>>(x, gt, out, H, W, normalize, make_taps<R1(), R2()>(sigma, rho));
  });
  if (!built) return sst_set_error(SST_ERR_UNSUPPORTED, "sst_st_maps: (sigma,rho)=(%g,%g) -> radii (%d,%d) not built", sigma, rho, r1, r2);
  SST_LAUNCH_CHECK("st_maps_kernel");
  return SST_OK;
}
