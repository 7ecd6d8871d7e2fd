// Tiled whole-image inference (upscale.py: Upscaler): the glue around the generator's forward.
//   sst_tile_gather    one LR image -> a batch of equal-size windows, fp32 NCHW, each transformed by one dihedral element t
//   sst_tile_scatter   the generator's output tiles -> each tile's OWNED rectangle into the fp32 CHW canvas, mapped back through the
//                      inverse of t; stored, or added (the eight passes of the self-ensemble)
//   sst_canvas_to_u8   canvas -> uint8 HWC/RGB with utils.tensor2img's quantisation
// The generator does all the arithmetic; these kernels move each byte once and are bound by memory traffic.
//
// Gather and scatter are one copy: out = dihedral(window of a source, t) restricted to a rectangle of `out`, with
//   t = 4*transpose + 2*vflip + 1*hflip, applied in that order (device_data.dihedral):
//   out[y][x] = win[sy][sx],  y' = t&2 ? Ho-1-y : y,  x' = t&1 ? Wo-1-x : x,  (sy, sx) = t&4 ? (x', y') : (y', x')
// (Ho x Wo: the shape of `out`, i.e. the window's shape, swapped when t&4).  The gather copies whole windows of the image into
// packed tiles; the scatter copies, from a tile taken as the source, the rectangle that the tile owns to its place in the canvas
// with the inverse element t^-1 (upscale.inverse_dihedral; dihedral(dihedral(x, t), t^-1) == x).
//
// One workgroup per (tile, TY x TX rectangle of `out`).  It stages the source pixels of its rectangle in LDS with reads that run
// along source rows - rows of TX pixels without transpose, TX rows of TY pixels with it (TY = 32 then, so that a row's share is
// 128 B of fp32) - and stores rows of `out`, consecutive lanes at consecutive x.  Call the source axis that y' walks the MAJOR axis
// and the one x' walks the MINOR axis: the transpose is only the choice of the two LDS strides, both flips are index maps of the
// reader.  LDS rows have an odd number of dwords, so lanes that walk the row index (the transposed read) spread over the banks.
// A uint8 source is HWC: a window row starts at byte 3*x0 of an image row of 3*W bytes, no alignment at all, so every staged dword
// is funnel-shifted from the aligned dwords that hold its bytes (pixel_io.h); the image sits at a 16-byte aligned base in a buffer
// padded to a multiple of 16 bytes.  Every offset into an image, a tile batch or the canvas is 64-bit.
//
// Each workgroup checks its tile's descriptor again (the host has checked what it can see; the tables live on the device): a
// gather row outside the image yields NaN for that tile, a scatter row outside the image or the window is skipped; neither reads
// the source.
#include "common.h"
#include "pixel_io.h"

namespace {

constexpr int TILE_NT = 256;
constexpr int TILE_TX = 64;                       // columns of `out` per workgroup
constexpr int TILE_TY = 16, TILE_TY_TR = 32;      // rows of `out` per workgroup, without / with transpose
constexpr int TILE_LDS = 3 * TILE_TX * (TILE_TY_TR + 1);   // dwords: fp32, transposed: 3 planes x 64 rows x 33 (the largest case)
static_assert(3 * TILE_TY * (TILE_TX + 1) <= TILE_LDS, "fp32, no transpose: 3 planes x 16 rows x 65 dwords");
static_assert(TILE_TY * (3 * TILE_TX / 4 + 1) <= TILE_LDS && TILE_TX * (3 * TILE_TY_TR / 4 + 1) <= TILE_LDS, "uint8 rows");

__host__ __device__ inline int tile_ty(int t) { return (t & 4) ? TILE_TY_TR : TILE_TY; }

// out[y][x] = dihedral(win, t)[y][x] for y in [y0, y1), x in [x0, x1)  (y1 - y0 <= tile_ty(t), x1 - x0 <= TILE_TX), three channels.
// win: the window at (wy0, wx0) of the source - U8: HWC bytes, rows of SW pixels; else CHW floats, rows of SW, planes of `plane`.
// Ho x Wo: the shape of dihedral(win, t).  dst points at out(c = 0, y0, x0); channel planes `dplane` apart, rows `dpitch`.
// The caller guarantees that the window is inside the source.  All threads of the workgroup call it.
template <bool U8>
__device__ __forceinline__ void dihedral_copy(const void* __restrict__ src, int64_t plane, int SW, int wy0, int wx0, int t, int Ho,
                                              int Wo, int y0, int y1, int x0, int x1, float* __restrict__ dst, int64_t dplane,
                                              int64_t dpitch, bool accumulate, const float* s_lut, uint32_t* s_buf) {
  const int tid = threadIdx.x;
  const bool tr = t & 4, vf = t & 2, hf = t & 1;
  const int rows = y1 - y0, cols = x1 - x0;
  const int lo = vf ? Ho - y1 : y0, xlo = hf ? Wo - x1 : x0;      // first major line / first minor index of the rectangle
  const int nrow = tr ? cols : rows;                              // source rows read
  const int seg = tr ? rows : cols;                               // pixels of each
  const int64_t sy0 = (int64_t)wy0 + (tr ? xlo : lo), sx0 = (int64_t)wx0 + (tr ? lo : xlo);
  int P;                                                          // dwords per LDS row, odd
  if (U8) {
    const int segb = 3 * seg, ndw = (segb + 3) >> 2;
    P = ndw | 1;
    const uint8_t* s8 = static_cast<const uint8_t*>(src);
    const int64_t base = (sy0 * SW + sx0) * 3, rowb = (int64_t)SW * 3;
    for (int i = tid; i < nrow * ndw; i += TILE_NT) {
      const int row = i / ndw, k = i - row * ndw;
      s_buf[row * P + k] = load_dword_unaligned(s8, base + row * rowb + 4 * k, min(4, segb - 4 * k));
    }
  } else {
    P = seg | 1;
    const float* sf = static_cast<const float*>(src);
    float* s_f = reinterpret_cast<float*>(s_buf);
    for (int i = tid; i < 3 * nrow * seg; i += TILE_NT) {
      const int k = i % seg, rc = i / seg, row = rc % nrow, c = rc / nrow;
      s_f[rc * P + k] = sf[c * plane + (sy0 + row) * SW + sx0 + k];
    }
  }
  __syncthreads();
  const uint8_t* s_b = reinterpret_cast<const uint8_t*>(s_buf);
  const float* s_f = reinterpret_cast<const float*>(s_buf);
  for (int i = tid; i < 3 * rows * cols; i += TILE_NT) {
    const int x = i % cols, rc = i / cols, r = rc % rows, c = rc / rows;
    const int line = (vf ? Ho - 1 - (y0 + r) : y0 + r) - lo, xm = (hf ? Wo - 1 - (x0 + x) : x0 + x) - xlo;
    const int row = tr ? xm : line, k = tr ? line : xm;
    const float v = U8 ? s_lut[s_b[row * (P * 4) + k * 3 + c]] : s_f[(c * nrow + row) * P + k];
    float* o = dst + c * dplane + r * dpitch + x;
    *o = accumulate ? *o + v : v;
  }
}

// rectangle (ty, tx) of an h x w area, in area coordinates
__device__ __forceinline__ bool sub_rect(int idx, int h, int w, int TY, int& y0, int& y1, int& x0, int& x1) {
  const int ntx = (w + TILE_TX - 1) / TILE_TX;
  const int ty = idx / ntx, tx = idx - ty * ntx;
  y0 = ty * TY, x0 = tx * TILE_TX;
  if (y0 >= h) return false;
  y1 = min(y0 + TY, h), x1 = min(x0 + TILE_TX, w);
  return true;
}

template <bool U8>
__global__ __launch_bounds__(TILE_NT) void tile_gather_kernel(const void* __restrict__ src, int H, int W, const int* __restrict__ desc,
                                                              int th, int tw, int t, const float* __restrict__ lut,
                                                              float* __restrict__ out) {
  __shared__ __align__(16) uint32_t s_buf[TILE_LDS];
  __shared__ float s_lut[U8 ? 256 : 1];
  const int b = blockIdx.y;
  const int Ho = (t & 4) ? tw : th, Wo = (t & 4) ? th : tw;
  int y0, y1, x0, x1;
  if (!sub_rect(blockIdx.x, Ho, Wo, tile_ty(t), y0, y1, x0, x1)) return;
  float* dst = out + ((int64_t)b * 3 * Ho + y0) * Wo + x0;
  const int64_t dplane = (int64_t)Ho * Wo;
  const int wy0 = desc[3 * b], wx0 = desc[3 * b + 1];
  const bool ok = desc[3 * b + 2] == t && wy0 >= 0 && wx0 >= 0 && (int64_t)wy0 + th <= H && (int64_t)wx0 + tw <= W;
  if (!ok) {      // the host checks the table it is given; a row that still gets here yields NaN, never a stray read
    const float q = __builtin_nanf("");
    const int rows = y1 - y0, cols = x1 - x0;
    for (int i = threadIdx.x; i < 3 * rows * cols; i += TILE_NT) {
      const int x = i % cols, rc = i / cols;
      dst[(rc / rows) * dplane + (int64_t)(rc % rows) * Wo + x] = q;
    }
    return;
  }
  if (U8) s_lut[threadIdx.x] = lut[threadIdx.x];                      // TILE_NT == 256; dihedral_copy syncs before it reads
  dihedral_copy<U8>(src, (int64_t)H * W, W, wy0, wx0, t, Ho, Wo, y0, y1, x0, x1, dst, dplane, Wo, false, s_lut, s_buf);
}

// tiles [B,3,s*th',s*tw'] -> canvas [3,s*H,s*W]; rows [B,6] = (y0, x0, oy0, oy1, ox0, ox1) in LR pixels; tinv = the inverse of the
// element the tiles were gathered with.  The grid covers the largest rectangle a tile can own (the whole window).
__global__ __launch_bounds__(TILE_NT) void tile_scatter_kernel(const float* __restrict__ tiles, const int* __restrict__ rows, int H,
                                                               int W, int th, int tw, int s, int tinv, float* __restrict__ canvas,
                                                               int accumulate) {
  __shared__ __align__(16) uint32_t s_buf[TILE_LDS];
  const int b = blockIdx.y;
  const int* r = rows + 6 * b;
  const int wy0 = r[0], wx0 = r[1], oy0 = r[2], oy1 = r[3], ox0 = r[4], ox1 = r[5];
  const bool ok = wy0 >= 0 && wx0 >= 0 && (int64_t)wy0 + th <= H && (int64_t)wx0 + tw <= W && oy0 >= wy0 && oy0 < oy1 &&
                  oy1 <= wy0 + th && ox0 >= wx0 && ox0 < ox1 && ox1 <= wx0 + tw;
  if (!ok) return;                                                    // nothing is touched for a row that is out of range
  int y0, y1, x0, x1;                                                 // in the owned rectangle's coordinates
  if (!sub_rect(blockIdx.x, s * (oy1 - oy0), s * (ox1 - ox0), tile_ty(tinv), y0, y1, x0, x1)) return;
  const int Ho = s * th, Wo = s * tw;                                 // the tile in the canvas's orientation
  const int ey = s * (oy0 - wy0), ex = s * (ox0 - wx0);               // the owned rectangle's origin in it
  const int64_t sW = (int64_t)s * W, dplane = (int64_t)s * H * sW;
  float* dst = canvas + ((int64_t)s * oy0 + y0) * sW + (int64_t)s * ox0 + x0;
  const int SW = (tinv & 4) ? Ho : Wo;                                // row length of the tile as the generator wrote it
  dihedral_copy<false>(tiles + (int64_t)b * 3 * Ho * Wo, (int64_t)Ho * Wo, SW, 0, 0, tinv, Ho, Wo, ey + y0, ey + y1, ex + x0, ex + x1,
                       dst, dplane, sW, accumulate != 0, nullptr, s_buf);
}

// four pixels per thread: three float4 loads (one per plane) when the planes are 16-byte aligned, twelve bytes out
__global__ __launch_bounds__(256) void canvas_to_u8_kernel(const float* __restrict__ canvas, int64_t n, float scale,
                                                            uint8_t* __restrict__ out, int vec) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, p0 = g * 4;
  if (p0 >= n) return;
  const int m = (int)min((int64_t)4, n - p0);
  uint8_t q[12];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const float* p = canvas + c * n + p0;
    if (vec) {
      const float4 f = *reinterpret_cast<const float4*>(p);
      v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < m) v[j] = p[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) q[3 * j + c] = to_u8(quantise(v[j] * scale));
  }
  uint8_t* o = out + p0 * 3;
  if (m == 4) {
    uint32_t w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = q[4 * k] | (q[4 * k + 1] << 8) | (q[4 * k + 2] << 16) | ((uint32_t)q[4 * k + 3] << 24);
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);                    // byte 12*g of a 4-byte aligned buffer
    o4[0] = w[0], o4[1] = w[1], o4[2] = w[2];
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j)
      if (j < 3 * m) o[j] = q[j];
  }
}

int sub_rects(int h, int w, int t) { return ((h + tile_ty(t) - 1) / tile_ty(t)) * ((w + TILE_TX - 1) / TILE_TX); }

}  // namespace

SST_API int sst_tile_gather(const uint8_t* src_u8, const float* src_f32, int64_t src_bytes, int H, int W, const int* desc, int B, int th,
                            int tw, int t, const float* lut, float* out, void* stream) {
  SST_REQUIRE((src_u8 != nullptr) != (src_f32 != nullptr), "sst_tile_gather: exactly one of the uint8 and the fp32 source must be given");
  SST_REQUIRE(desc && out && H > 0 && W > 0 && B > 0 && B <= 65535, "sst_tile_gather: bad argument (at most 65535 tiles)");
  SST_REQUIRE(t >= 0 && t < 8, "sst_tile_gather: t %d outside [0, 8)", t);
  SST_REQUIRE(th > 0 && tw > 0 && th <= H && tw <= W, "sst_tile_gather: window %dx%d does not fit the %dx%d image", tw, th, W, H);
  const int64_t need = (int64_t)H * W * 3 * (src_u8 ? 1 : 4);
  SST_REQUIRE(src_bytes >= need, "sst_tile_gather: the source buffer holds %lld bytes, the image needs %lld", (long long)src_bytes,
              (long long)need);
  if (src_u8)
    SST_REQUIRE(lut && (reinterpret_cast<uintptr_t>(src_u8) & 15) == 0 && src_bytes % 16 == 0,
                "sst_tile_gather: the uint8 image needs the LUT, a 16-byte aligned base and a buffer padded to a multiple of 16 bytes "
                "(%lld)", (long long)src_bytes);
  const int Ho = (t & 4) ? tw : th, Wo = (t & 4) ? th : tw;
  const int64_t nsub = (int64_t)sub_rects(Ho, Wo, t);
  SST_REQUIRE(nsub < (1ll << 31), "sst_tile_gather: window too large");
  const dim3 grid((unsigned)nsub, B);
  if (src_u8)
    tile_gather_kernel<true><<<grid, TILE_NT, 0, sst_stream(stream)>>>(src_u8, H, W, desc, th, tw, t, lut, out);
  else
    tile_gather_kernel<false><<<grid, TILE_NT, 0, sst_stream(stream)>>>(src_f32, H, W, desc, th, tw, t, lut, out);
  SST_LAUNCH_CHECK("tile_gather_kernel");
  return SST_OK;
}

SST_API int sst_tile_scatter(const float* tiles, const int* rows, int B, int H, int W, int th, int tw, int scale, int t, float* canvas,
                             int accumulate, void* stream) {
  SST_REQUIRE(tiles && rows && canvas && H > 0 && W > 0 && B > 0 && B <= 65535, "sst_tile_scatter: bad argument (at most 65535 tiles)");
  SST_REQUIRE(t >= 0 && t < 8, "sst_tile_scatter: t %d outside [0, 8)", t);
  SST_REQUIRE(th > 0 && tw > 0 && th <= H && tw <= W, "sst_tile_scatter: window %dx%d does not fit the %dx%d image", tw, th, W, H);
  SST_REQUIRE(scale >= 1 && scale <= 8 && (int64_t)scale * th < (1 << 24) && (int64_t)scale * tw < (1 << 24),
              "sst_tile_scatter: scale %d outside [1, 8] or window too large", scale);
  const int tinv = t < 4 ? t : (4 | ((t & 1) << 1) | ((t & 2) >> 1));     // upscale.inverse_dihedral
  const int64_t nsub = (int64_t)sub_rects(scale * th, scale * tw, tinv);
  SST_REQUIRE(nsub < (1ll << 31), "sst_tile_scatter: window too large");
  tile_scatter_kernel<<<dim3((unsigned)nsub, B), TILE_NT, 0, sst_stream(stream)>>>(tiles, rows, H, W, th, tw, scale, tinv, canvas,
                                                                                  accumulate);
  SST_LAUNCH_CHECK("tile_scatter_kernel");
  return SST_OK;
}

SST_API int sst_canvas_to_u8(const float* canvas, int H, int W, float scale, uint8_t* out, void* stream) {
  SST_REQUIRE(canvas && out && H > 0 && W > 0, "sst_canvas_to_u8: bad argument");
  SST_REQUIRE(scale == 1.f || scale == 0.125f, "sst_canvas_to_u8: scale must be 1 or 0.125 (one pass or the mean of eight)");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "sst_canvas_to_u8: the output must be 4-byte aligned");
  const int64_t n = (int64_t)H * W, groups = (n + 3) / 4, blocks = (groups + 255) / 256;
  SST_REQUIRE(blocks < (1ll << 31), "sst_canvas_to_u8: image too large");
  const int vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(canvas) & 15) == 0;
  canvas_to_u8_kernel<<<(unsigned)blocks, 256, 0, sst_stream(stream)>>>(canvas, n, scale, out, vec);
  SST_LAUNCH_CHECK("canvas_to_u8_kernel");
  return SST_OK;
}
