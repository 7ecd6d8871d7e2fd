// Batch gather from an HBM-resident uint8 crop store (device_data.py: DeviceImageSet / DeviceLoader).  One launch builds a
// training batch: the crops named by idx are gathered from src [N,H,W,3] (HWC/RGB uint8, as read_image decodes them), turned into
// fp32 NCHW on the 1/255 grid through a host-made LUT (gt = lut[u], bit-identical to u8.float() / 255), and the x1/s LR is
// synthesised from them in the same launch with bicubic.py's tap tables - the arithmetic of misc.hip:bicubic_kernel, term for term:
//   V[x] = sum_ty wy[oy][ty] * gt[iy[oy][ty]][x]  (ty in table order, v += in * wy)
//   lr[oy][ox] = rint(255 * sum_tx wx[ox][tx] * V[ix[ox][tx]]) / 255  (tx in table order, acc += v * wx)
// so lr equals Bicubic("cuda")(gt) bit for bit.
//
// One workgroup per (image, band of HR rows).  With lr the bands are the LR rows (band oy = HR rows [oy*H/oh, (oy+1)*H/oh)); the
// workgroup stages in LDS, as raw bytes, the Ty HR rows its LR row's taps name (iy, clamped at the borders, so a row may repeat) and
// its own band rows, with 16-byte loads where the rows are 16-byte aligned (W % 16 == 0: every 96- / 192-px crop).  gt is written
// from the band rows with float4 stores per channel plane; the vertical bicubic pass reads the tap rows from LDS into one row of
// column sums V (LDS, fp32, HWC order) and the horizontal pass reads V.  LDS: 1 KiB LUT + 12*W B of V + (Ty + band) * 3W B
// (192 px, x1/8: about 28 KiB).
#include "common.h"

namespace {

constexpr int GATHER_NT = 256;

__device__ __forceinline__ void stage_row(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int W3, bool vec, int lane0,
                                          int step) {
  if (vec) {
    const int n16 = W3 >> 4;
    for (int k = lane0; k < n16; k += step)
      reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(src)[k];
  } else {
    for (int k = lane0; k < W3; k += step) dst[k] = src[k];
  }
}

__global__ __launch_bounds__(GATHER_NT) void gather_batch_kernel(
    const uint8_t* __restrict__ src, int64_t N, const int* __restrict__ idx, int H, int W, int nband,
    const float* __restrict__ lut, float* __restrict__ gt, float* __restrict__ lr, const float* __restrict__ wy,
    const int* __restrict__ iy, const float* __restrict__ wx, const int* __restrict__ ix, int oh, int ow, int Ty, int Tx,
    int band_max, int vec) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
  const int W3 = W * 3;
  const int W3p = (W3 + 15) & ~15;
  float* s_lut = reinterpret_cast<float*>(smem);                         // [256]
  float* s_v = s_lut + 256;                                              // [W3p] column sums of the vertical pass
  uint8_t* s_tap = reinterpret_cast<uint8_t*>(s_v + W3p);                // [Ty][W3p]   (lr only)
  uint8_t* s_band = s_tap + (lr ? (int64_t)Ty * W3p : 0);                // [band_max][W3p]   (gt only)
  const int y0 = (int)((int64_t)band * H / nband), y1 = (int)((int64_t)(band + 1) * H / nband);
  const int64_t n = idx[b];
  if (n < 0 || n >= N) {       // the host checks the index range; an index that still gets here yields NaN, never a stray read
    const float q = __builtin_nanf("");
    if (gt)
      for (int i = tid; i < 3 * (y1 - y0) * W; i += GATHER_NT) {
        const int x = i % W, r = i / W;
        gt[(((int64_t)b * 3 + r / (y1 - y0)) * H + y0 + r % (y1 - y0)) * W + x] = q;
      }
    if (lr)
      for (int i = tid; i < 3 * ow; i += GATHER_NT) lr[(((int64_t)b * 3 + i / ow) * oh + band) * ow + i % ow] = q;
    return;
  }
  const uint8_t* img = src + n * H * (int64_t)W3;
  s_lut[tid] = lut[tid];                                                 // GATHER_NT == 256

  // ---- stage: one wave per row, 16 B per lane (a 96-px row is 288 B = 18 lanes, a 192-px row 36 lanes)
  const int wave = tid >> 6, lane = tid & 63, nwave = GATHER_NT / 64;
  if (lr)
    for (int t = wave; t < Ty; t += nwave) stage_row(s_tap + t * W3p, img + (int64_t)iy[band * Ty + t] * W3, W3, vec, lane, 64);
  if (gt)
    for (int r = wave; r < y1 - y0; r += nwave) stage_row(s_band + r * W3p, img + (int64_t)(y0 + r) * W3, W3, vec, lane, 64);
  __syncthreads();

  // ---- gt: band rows -> NCHW planes, 4 pixels of one channel per float4 store
  if (gt) {
    const int rows = y1 - y0;
    if ((W & 3) == 0) {
      const int W4 = W >> 2;
      for (int i = tid; i < 3 * rows * W4; i += GATHER_NT) {
        const int x4 = i % W4, r = (i / W4) % rows, c = i / (W4 * rows);
        const uint8_t* p = s_band + r * W3p + x4 * 12 + c;
        const float4 v = make_float4(s_lut[p[0]], s_lut[p[3]], s_lut[p[6]], s_lut[p[9]]);
        *reinterpret_cast<float4*>(gt + (((int64_t)b * 3 + c) * H + y0 + r) * W + x4 * 4) = v;
      }
    } else {
      for (int i = tid; i < 3 * rows * W; i += GATHER_NT) {
        const int x = i % W, r = (i / W) % rows, c = i / (W * rows);
        gt[(((int64_t)b * 3 + c) * H + y0 + r) * W + x] = s_lut[s_band[r * W3p + x * 3 + c]];
      }
    }
  }
  if (!lr) return;

  // ---- lr, vertical pass: V[x*3 + c] = sum_ty gt[iy[ty]][c][x] * wy[ty]   (bicubic_kernel's inner loop, same order)
  const float* wrow = wy + band * Ty;
  for (int j = tid; j < W3; j += GATHER_NT) {
    float v = 0.f;
    for (int ty = 0; ty < Ty; ++ty) v += s_lut[s_tap[ty * W3p + j]] * wrow[ty];
    s_v[j] = v;
  }
  __syncthreads();
  // ---- horizontal pass: acc = sum_tx V[ix[tx]] * wx[tx], rounded to the 1/255 grid
  for (int i = tid; i < 3 * ow; i += GATHER_NT) {
    const int ox = i % ow, c = i / ow;
    float acc = 0.f;
    for (int tx = 0; tx < Tx; ++tx) acc += s_v[ix[ox * Tx + tx] * 3 + c] * wx[ox * Tx + tx];
    lr[(((int64_t)b * 3 + c) * oh + band) * ow + ox] = rintf(255.f * acc) / 255.f;
  }
}

}  // namespace

SST_API int sst_gather_batch(const uint8_t* src, int64_t N, const int* idx, int B, int H, int W, const float* lut, float* gt,
                             float* lr, const float* wy, const int* iy, const float* wx, const int* ix, int oh, int ow, int Ty,
                             int Tx, void* stream) {
  SST_REQUIRE(src && idx && lut && N > 0 && B > 0 && H > 0 && W > 0 && (gt || lr), "sst_gather_batch: bad argument");
  SST_REQUIRE(B <= 65535, "sst_gather_batch: batch %d > 65535", B);
  if (lr)
    SST_REQUIRE(wy && iy && wx && ix && oh > 0 && ow > 0 && oh <= H && ow <= W && Ty > 0 && Tx > 0,
                "sst_gather_batch: bad LR arguments");
  const int nband = lr ? oh : (H + 3) / 4;                       // gt only: bands of about four rows
  const int band_max = (H + nband - 1) / nband;
  const int W3p = (3 * W + 15) & ~15;
  const int64_t lds = 256 * 4 + (int64_t)W3p * 4 + (int64_t)((lr ? Ty : 0) + (gt ? band_max : 0)) * W3p;
  SST_REQUIRE(lds <= 64 * 1024, "sst_gather_batch: %lld B of LDS needed (H %d, W %d, Ty %d) > 64 KiB", (long long)lds, H, W, Ty);
  const int vec = (W * 3) % 16 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  gather_batch_kernel<<<dim3(nband, B), GATHER_NT, (size_t)lds, sst_stream(stream)>>>(src, N, idx, H, W, nband, lut, gt, lr, wy, iy,
                                                                                      wx, ix, oh, ow, Ty, Tx, band_max, vec);
  SST_LAUNCH_CHECK("gather_batch_kernel");
  return SST_OK;
}
