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

struct StMapsOut {
  float* Sx;
  float* Sgt;
  float* Fx;
  float* Fgt;
  float* d;
  float* tile_sums;
};

__device__ __forceinline__ void store_planes(float* __restrict__ out, size_t o, size_t hw, float v0, float v1, float v2) {
  out[o] = v0;
  out[o + hw] = v1;
  out[o + 2 * hw] = v2;
}

// (t, c2, s2) of one structure tensor
__device__ __forceinline__ void store_features(float* __restrict__ out, size_t o, size_t hw, float jxx, float jyy, float jxy) {
  const float t = jxx + jyy;
  const float den = t + 1e-12f;
  store_planes(out, o, hw, t, (jxx - jyy) / den, 2.f * jxy / den);
}

template <int R1, int R2>
__global__ __launch_bounds__(NT) void st_maps_kernel(const float* __restrict__ x, const float* __restrict__ gt, StMapsOut out, int H,
                                                     int W, int normalize, StTaps<R1, R2> tp) {
  __shared__ float lds[st_fwd_lds_floats<R1, R2>()];
  __shared__ float red[NT / 64];
  const int b = blockIdx.z, y0 = blockIdx.y * T, x0 = blockIdx.x * T;
  const size_t hw = (size_t)H * W, img_off = (size_t)b * 3 * hw;
  const bool want_d = out.d || out.tile_sums;
  const bool need1 = out.Sx || out.Fx || want_d, need2 = out.Sgt || out.Fgt || want_d;
  float J1[PPT][3] = {}, J2[PPT][3] = {};
  if (need1) tile_structure_tensor<R1, R2>(x + img_off, H, W, y0, x0, tp, lds, J1);
  if (need2) tile_structure_tensor<R1, R2>(gt + img_off, H, W, y0, x0, tp, lds, J2);

  float lsum = 0.f;
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int p = threadIdx.x + j * NT, y = y0 + (p >> 5), xx = x0 + (p & 31);
    if (y >= H || xx >= W) continue;                    // outside the image: neither stored nor summed
    const size_t px = (size_t)y * W + xx, o = img_off + px;
    if (out.Sx) store_planes(out.Sx, o, hw, J1[j][0], J1[j][1], J1[j][2]);
    if (out.Sgt) store_planes(out.Sgt, o, hw, J2[j][0], J2[j][1], J2[j][2]);
    if (out.Fx) store_features(out.Fx, o, hw, J1[j][0], J1[j][1], J1[j][2]);
    if (out.Fgt) store_features(out.Fgt, o, hw, J2[j][0], J2[j][1], J2[j][2]);
    if (want_d) {
      const float d = st_pointwise(J1[j][0], J1[j][1], J1[j][2], J2[j][0], J2[j][1], J2[j][2], normalize).d;
      if (out.d) out.d[(size_t)b * hw + px] = d;
      lsum += d;
    }
  }
  if (out.tile_sums) {                                  // uniform: every thread of every workgroup takes the same side
    const float bsum = block_sum<NT>(lsum, red);
    if (threadIdx.x == 0) out.tile_sums[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = bsum;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------ C ABI
SST_API int sst_st_maps_workspace(int B, int H, int W, int64_t* tile_floats) {
  SST_REQUIRE(B > 0 && H > 0 && W > 0 && tile_floats, "sst_st_maps_workspace: bad shape");
  *tile_floats = (int64_t)B * ((H + T - 1) / T) * ((W + T - 1) / T);
  return SST_OK;
}

SST_API int sst_st_maps(const float* x, const float* gt, float* Sx, float* Sgt, float* Fx, float* Fgt, float* d, float* tile_sums,
                        int B, int H, int W, float sigma, float rho, int normalize, void* stream) {
  SST_REQUIRE(x, "sst_st_maps: null pointer (x)");
  SST_REQUIRE(B > 0 && H > 0 && W > 0 && B <= 65535 && (H + T - 1) / T <= 65535, "sst_st_maps: bad shape B=%d H=%d W=%d", B, H, W);
  SST_REQUIRE(Sx || Sgt || Fx || Fgt || d || tile_sums, "sst_st_maps: no output requested");
  SST_REQUIRE(gt || !Sgt, "sst_st_maps: Sgt needs gt");
  SST_REQUIRE(gt || !Fgt, "sst_st_maps: Fgt needs gt");
  SST_REQUIRE(gt || !d, "sst_st_maps: d needs gt (the distance is between two images)");
  SST_REQUIRE(gt || !tile_sums, "sst_st_maps: tile_sums cannot be computed without gt (they are sums of d)");
  const int r1 = radius_of(sigma), r2 = radius_of(rho);
  const dim3 grid((W + T - 1) / T, (H + T - 1) / T, B);
  const StMapsOut out{Sx, Sgt, Fx, Fgt, d, tile_sums};
  if (r1 == 2 && r2 == 8) {
    st_maps_kernel<2, 8><<<grid, NT, 0, sst_stream(stream)>>>(x, gt, out, H, W, normalize, make_taps<2, 8>(sigma, rho));
  } else if (r1 == 4 && r2 == 10) {
    st_maps_kernel<4, 10><<<grid, NT, 0, sst_stream(stream)>>>(x, gt, out, H, W, normalize, make_taps<4, 10>(sigma, rho));
  } else {
    return sst_set_error(SST_ERR_UNSUPPORTED, "sst_st_maps: (sigma,rho)=(%g,%g) -> radii (%d,%d) not built", sigma, rho, r1, r2);
  }
  SST_LAUNCH_CHECK("st_maps_kernel");
  return SST_OK;
}
