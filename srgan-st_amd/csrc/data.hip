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
#include "pixel_io.h"      // load_dword_unaligned
#include "degrade.h"       // the degradation stage of gather_crops_degraded_kernel
#include <algorithm>

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


// ---- Batch gather from WHOLE images (device_data.py: DeviceImageArena / DeviceCropLoader): crop, dihedral transform, conversion
// and LR synthesis in one launch.  arena: packed HWC/RGB uint8 images; table [N,3] int64 = (byte offset, H_img, W_img) per image;
// desc [B,4] int32 = (image, y0, x0, t) per sample.  With C = img[y0:y0+S, x0:x0+S] and t = 4*transpose + 2*vflip + 1*hflip
// (applied in that order):   out[y][x] = C[sy][sx],  y' = t&2 ? S-1-y : y,  x' = t&1 ? S-1-x : x,  (sy,sx) = t&4 ? (x',y') : (y',x').
// gt = lut[out]; lr = the bicubic of OUT (not the transform of C's bicubic: fp32 sums are not order-symmetric), in the term order
// of gather_batch_kernel above, so lr equals Bicubic("cuda")(gt) bit for bit.
//
// One workgroup per (sample, band of output rows), as above.  Call the source axis that y' walks the MAJOR axis (source rows
// without transpose, source columns with it) and the one x' walks the MINOR axis.  The band's output rows and its LR row's taps
// name a run of consecutive major lines [lo, hi] (the taps are consecutive, clamped at the borders; hi - lo < span, the caller's
// bound, else NaN).  The workgroup stages exactly that run as raw bytes in source order:
//   no transpose: hi-lo+1 source rows of 3S bytes, LDS pitch W3p;         byte(line, x', c) at (line-lo)*W3p + x'*3 + c
//   transpose:    from each of the S source rows the 3*(hi-lo+1) bytes of columns lo..hi, coalesced along the source row, LDS
//                 pitch P (P/4 odd: lanes that walk x' spread over the banks);   byte(line, x', c) at x'*P + (line-lo)*3 + c
// so the transpose is only the choice of the two strides, and both flips are index maps of the consumers.  A crop row starts at
// byte 3*x0 of an image row of 3*W_img bytes: no alignment at all.  Every staged dword is therefore funnel-shifted from the one or
// two ALIGNED dwords that hold its bytes; an aligned dword that holds a byte of an image lies inside the arena (base and size are
// multiples of 16), so nothing outside the arena is read.  The vertical pass leaves the column sums V indexed by x' (each sum is
// one column's own, so its place in V changes no bit) and the horizontal pass reads V through the hflip map.
constexpr int CROPS_NT = 256;

// The sample of descriptor d = (image, y0, x0, t): every field checked here again (the host has checked them); false when anything
// is out of range.  off: the image's byte offset in the arena, Wi: its width.
__device__ __forceinline__ bool crop_sample(const int4 d, const int64_t* __restrict__ table, int64_t N, int64_t arena_bytes, int S,
                                            int64_t& off, int64_t& Wi) {
  bool ok = d.x >= 0 && d.x < N && d.w >= 0 && d.w < 8;
  if (ok) {
    off = table[(int64_t)d.x * 3], Wi = table[(int64_t)d.x * 3 + 2];
    const int64_t Hi = table[(int64_t)d.x * 3 + 1];
    ok = off >= 0 && off <= arena_bytes && Hi > 0 && Wi > 0 && Wi <= arena_bytes && Hi <= (arena_bytes - off) / (3 * Wi) &&
         d.y >= 0 && d.z >= 0 && (int64_t)d.y + S <= Hi && (int64_t)d.z + S <= Wi;
  }
  return ok;
}

// Stage the major lines [lo, lo + nline) of the sample's window as raw bytes (layout: above); consecutive lanes take consecutive
// dwords of a source row's segment.
__device__ __forceinline__ void stage_lines(const uint8_t* __restrict__ arena, uint8_t* __restrict__ s_src, int64_t off, int64_t Wi,
                                            const int4 d, bool tr, int lo, int nline, int S, int W3p, int P) {
  const int nrow = tr ? S : nline;                                       // source rows read
  const int seg = tr ? nline * 3 : S * 3;                                // bytes of each
  const int pitch = tr ? P : W3p;
  const int ndw = (seg + 3) >> 2;
  const int64_t base = off + (((int64_t)d.y + (tr ? 0 : lo)) * Wi + d.z + (tr ? lo : 0)) * 3;
  const int64_t rowb = Wi * 3;
  uint32_t* dst = reinterpret_cast<uint32_t*>(s_src);
  for (int i = threadIdx.x; i < nrow * ndw; i += CROPS_NT) {
    const int row = i / ndw, k = i - row * ndw;
    dst[row * (pitch >> 2) + k] = load_dword_unaligned(arena, base + row * rowb + 4 * k, min(4, seg - 4 * k));
  }
}

__global__ __launch_bounds__(CROPS_NT) void gather_crops_kernel(
    const uint8_t* __restrict__ arena, int64_t arena_bytes, const int64_t* __restrict__ table, int64_t N,
    const int* __restrict__ desc, int S, int nband, const float* __restrict__ lut, float* __restrict__ gt, float* __restrict__ lr,
    const float* __restrict__ wy, const int* __restrict__ iy, const float* __restrict__ wx, const int* __restrict__ ix, int oh,
    int ow, int Ty, int Tx, int span, int P) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
  const int S3 = S * 3;
  const int W3p = (S3 + 15) & ~15;
  float* s_lut = reinterpret_cast<float*>(smem);                         // [256]
  float* s_v = s_lut + 256;                                              // [W3p] column sums of the vertical pass, indexed by x'
  uint8_t* s_src = reinterpret_cast<uint8_t*>(s_v + W3p);                // the staged run of major lines (see above)
  const int yb0 = (int)((int64_t)band * S / nband), yb1 = (int)((int64_t)(band + 1) * S / nband);

  // ---- the sample: every field checked here again (the host has checked them); anything out of range yields NaN below
  const int4 d = reinterpret_cast<const int4*>(desc)[b];
  const int t = d.w;
  const bool tr = t & 4, vf = t & 2, hf = t & 1;
  int64_t off = 0, Wi = 0;
  bool ok = crop_sample(d, table, N, arena_bytes, S, off, Wi);
  // ---- the run [lo, hi] of major lines this band needs
  int lo = S, hi = -1;
  if (gt) {
    const int m0 = vf ? S - 1 - yb0 : yb0, m1 = vf ? S - yb1 : yb1 - 1;
    lo = min(m0, m1), hi = max(m0, m1);
  }
  if (lr)
    for (int ty = 0; ty < Ty; ++ty) {
      const int r = iy[band * Ty + ty];
      ok = ok && r >= 0 && r < S;
      const int m = vf ? S - 1 - r : r;
      lo = min(lo, m), hi = max(hi, m);
    }
  const int nline = hi - lo + 1;
  ok = ok && nline >= 1 && nline <= span;
  if (!ok) {
    const float q = __builtin_nanf("");
    if (gt)
      for (int i = tid; i < 3 * (yb1 - yb0) * S; i += CROPS_NT) {
        const int x = i % S, r = i / S;
        gt[(((int64_t)b * 3 + r / (yb1 - yb0)) * S + yb0 + r % (yb1 - yb0)) * S + x] = q;
      }
    if (lr)
      for (int i = tid; i < 3 * ow; i += CROPS_NT) lr[(((int64_t)b * 3 + i / ow) * oh + band) * ow + i % ow] = q;
    return;
  }
  s_lut[tid] = lut[tid];                                                 // CROPS_NT == 256

  // ---- stage: consecutive lanes take consecutive dwords of a source row's segment
  stage_lines(arena, s_src, off, Wi, d, tr, lo, nline, S, W3p, P);
  __syncthreads();
  const int sL = tr ? 3 : W3p, sX = tr ? P : 3;                          // byte(line, x', c) = s_src[(line - lo) * sL + x' * sX + c]

  // ---- gt: the band's output rows -> NCHW planes, 4 pixels of one channel per float4 store  (S % 4 == 0)
  if (gt) {
    const int rows = yb1 - yb0, S4 = S >> 2;
    for (int i = tid; i < 3 * rows * S4; i += CROPS_NT) {
      const int x4 = i % S4, r = (i / S4) % rows, c = i / (S4 * rows);
      const int y = yb0 + r, x = x4 * 4;
      const uint8_t* p = s_src + ((vf ? S - 1 - y : y) - lo) * sL + (hf ? S - 1 - x : x) * sX + c;
      const int dx = hf ? -sX : sX;
      const float4 v = make_float4(s_lut[p[0]], s_lut[p[dx]], s_lut[p[2 * dx]], s_lut[p[3 * dx]]);
      *reinterpret_cast<float4*>(gt + (((int64_t)b * 3 + c) * S + y) * S + x) = v;
    }
  }
  if (!lr) return;

  // ---- lr, vertical pass: V[x'*3 + c] = sum_ty out[iy[ty]][c][x] * wy[ty]   (bicubic_kernel's inner loop, same order)
  const float* wrow = wy + band * Ty;
  const int* irow = iy + band * Ty;
  for (int j = tid; j < S3; j += CROPS_NT) {
    const int xs = j / 3, c = j - xs * 3;
    const uint8_t* p = s_src + xs * sX + c;
    float v = 0.f;
    for (int ty = 0; ty < Ty; ++ty) {
      const int r = irow[ty];
      v += s_lut[p[((vf ? S - 1 - r : r) - lo) * sL]] * wrow[ty];
    }
    s_v[j] = v;
  }
  __syncthreads();
  // ---- horizontal pass: acc = sum_tx V[x'(ix[tx])] * wx[tx], rounded to the 1/255 grid
  for (int i = tid; i < 3 * ow; i += CROPS_NT) {
    const int ox = i % ow, c = i / ow;
    float acc = 0.f;
    for (int tx = 0; tx < Tx; ++tx) {
      const int x = min(max(ix[ox * Tx + tx], 0), S - 1);
      acc += s_v[(hf ? S - 1 - x : x) * 3 + c] * wx[ox * Tx + tx];
    }
    lr[(((int64_t)b * 3 + c) * oh + band) * ow + ox] = rintf(255.f * acc) / 255.f;
  }
}


// ---- The same gather with the degradation stage of degrade.h between the conversion and the LR (DATA.DEGRADE): per sample a blur
// with its own Gaussian kernel, the bicubic, noise, quantise; gt as above.  One workgroup per (sample, band of R <= deg::ROWS_MAX LR
// rows, channel): the blur is K*K FMAs per pixel, so the channels are spread over workgroups (each stages the band's bytes for
// itself: 12 KiB against 0.85 M FMAs at S = 96, K = 21) and a band of R LR rows blurs (R - 1) * scale + Ty rows for the R * scale it
// owns (R = 2, x4: 20 for 8) instead of Ty for scale (16 for 4).  The band's taps name the blur rows [lo_b, hi_b] of the OUTPUT
// (transformed) crop; those, p = K / 2 rows of reflected halo on either side (reflected at the crop's border: rows
// [max(0, lo_b - p), min(S - 1, hi_b + p)], a contiguous run, as p < S) and the band's own rows are staged as the major lines
// [lo, hi] exactly as above.  The channel's fp32 plane is then built ONCE from the bytes, in output orientation and with the halo
// laid out (deg::finish_tile's input), so both flips, the transposition and the reflection are index maps of that one pass.
__global__ __launch_bounds__(deg::NT) void gather_crops_degraded_kernel(
    const uint8_t* __restrict__ arena, int64_t arena_bytes, const int64_t* __restrict__ table, int64_t N,
    const int* __restrict__ desc, int S, const float* __restrict__ lut, float* __restrict__ gt, float* __restrict__ lr,
    const float* __restrict__ wy, const int* __restrict__ iy, const float* __restrict__ wx, const int* __restrict__ ix, int oh,
    int ow, int Ty, int Tx, const int* __restrict__ dg, int K, int quantise, int R, int nr_max, int nline_max, int P) {
  static_assert(CROPS_NT == deg::NT, "stage_lines and the degradation stage run with one workgroup size");
  extern __shared__ __align__(16) unsigned char smem[];
  const int b = blockIdx.y, band = blockIdx.x / 3, c = blockIdx.x % 3, tid = threadIdx.x;
  const int W3p = (S * 3 + 15) & ~15;
  const int64_t raw = (int64_t)nline_max * W3p > (int64_t)S * P ? (int64_t)nline_max * W3p : (int64_t)S * P;
  const deg::Layout L(K, R, nr_max, S, raw, 256 * 4);
  const int p = L.p;
  uint8_t* s_src = smem + L.o_a;                                         // the staged run of major lines; later the blurred tile
  float* s_lut = reinterpret_cast<float*>(smem + L.o_tail);              // [256]
  deg::Tile tl;
  tl.oy0 = band * R, tl.noy = min(R, oh - tl.oy0), tl.ox0 = 0, tl.nox = ow, tl.c0 = 0, tl.nc = S;
  const int yb0 = (int)((int64_t)tl.oy0 * S / oh), yb1 = (int)((int64_t)(tl.oy0 + tl.noy) * S / oh);
  float* lr_plane = lr + ((int64_t)b * 3 + c) * oh * ow;

  const int4 d = reinterpret_cast<const int4*>(desc)[b];
  const int t = d.w;
  const bool tr = t & 4, vf = t & 2, hf = t & 1;
  int64_t off = 0, Wi = 0;
  bool ok = crop_sample(d, table, N, arena_bytes, S, off, Wi);
  // ---- the blur rows [lo_b, hi_b], then the run [lo, hi] of major lines: those with their halo, and with gt the band's own rows
  int hi_b;
  ok = deg::tap_rows(iy, Ty, tl.oy0, tl.noy, S, tl.r0, hi_b) && ok;
  tl.nr = hi_b - tl.r0 + 1;
  int y_lo = max(0, tl.r0 - p), y_hi = min(S - 1, hi_b + p);
  if (gt) y_lo = min(y_lo, yb0), y_hi = max(y_hi, yb1 - 1);
  const int lo = vf ? S - 1 - y_hi : y_lo, hi = vf ? S - 1 - y_lo : y_hi;
  const int nline = hi - lo + 1;
  ok = ok && tl.nr <= nr_max && nline >= 1 && nline <= nline_max;
  if (!ok) {
    const float q = __builtin_nanf("");
    if (gt)
      for (int i = tid; i < (yb1 - yb0) * S; i += deg::NT) gt[(((int64_t)b * 3 + c) * S + yb0 + i / S) * S + i % S] = q;
    return deg::fill_nan(lr_plane, tl, ow);
  }
  const deg::Params q = deg::load_params(dg, b);
  s_lut[tid] = lut[tid];                                                 // deg::NT == 256
  if (q.blur()) deg::weights_raw(reinterpret_cast<float*>(smem + L.o_k), q, K);
  stage_lines(arena, s_src, off, Wi, d, tr, lo, nline, S, W3p, P);
  __syncthreads();
  if (q.blur() && tid == deg::NT - 1)                                   // one thread, beside the others' gt and plane passes
    deg::weights_sum(reinterpret_cast<const float*>(smem + L.o_k), reinterpret_cast<double*>(smem), K);
  const int sL = tr ? 3 : W3p, sX = tr ? P : 3;                          // byte(line, x', c) = s_src[(line - lo) * sL + x' * sX + c]

  // ---- gt: this channel's plane of the band's output rows, 4 pixels per float4 store  (S % 4 == 0)
  if (gt) {
    const int rows = yb1 - yb0, S4 = S >> 2;
    for (int i = tid; i < rows * S4; i += deg::NT) {
      const int x4 = i % S4, y = yb0 + i / S4, x = x4 * 4;
      const uint8_t* s = s_src + ((vf ? S - 1 - y : y) - lo) * sL + (hf ? S - 1 - x : x) * sX + c;
      const int dx = hf ? -sX : sX;
      const float4 v = make_float4(s_lut[s[0]], s_lut[s[dx]], s_lut[s[2 * dx]], s_lut[s[3 * dx]]);
      *reinterpret_cast<float4*>(gt + (((int64_t)b * 3 + c) * S + y) * S + x) = v;
    }
  }
  // ---- the plane: plane[r][j] = out[refl(lo_b - p + r)][refl(j - p)], each byte converted once
  float* plane = reinterpret_cast<float*>(smem + L.o_plane);
  const int wp = S + 2 * p;
  for (int i = tid; i < (tl.nr + 2 * p) * wp; i += deg::NT) {
    const int r = i / wp, j = i - r * wp;
    const int y = deg::refl(tl.r0 - p + r, S), x = deg::refl(j - p, S);
    plane[r * L.pitch + j] = s_lut[s_src[((vf ? S - 1 - y : y) - lo) * sL + (hf ? S - 1 - x : x) * sX + c]];
  }
  __syncthreads();
  deg::finish_tile(smem, L, tl, q, K, quantise, lr_plane, (uint32_t)c * (uint32_t)(oh * ow), wy, iy, wx, ix, ow, Ty, Tx);
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

SST_API int sst_gather_crops(const uint8_t* arena, int64_t arena_bytes, const int64_t* table, int64_t N, const int* desc, int B,
                             int S, const float* lut, float* gt, float* lr, const float* wy, const int* iy, const float* wx,
                             const int* ix, int oh, int ow, int Ty, int Tx, int span, void* stream) {
  SST_REQUIRE(arena && table && desc && lut && arena_bytes > 0 && N > 0 && B > 0 && S > 0 && (gt || lr),
              "sst_gather_crops: bad argument");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(arena) & 15) == 0 && arena_bytes % 16 == 0,
              "sst_gather_crops: the arena and its size (%lld B) must be multiples of 16 bytes", (long long)arena_bytes);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(desc) & 15) == 0, "sst_gather_crops: desc must be 16-byte aligned");
  SST_REQUIRE(B <= 65535, "sst_gather_crops: batch %d > 65535", B);
  SST_REQUIRE(S % 4 == 0 && S <= 16384, "sst_gather_crops: crop side %d must be a multiple of 4 (and at most 16384)", S);
  SST_REQUIRE(span > 0 && span <= S, "sst_gather_crops: span %d outside [1, %d]", span, S);
  if (lr)
    SST_REQUIRE(wy && iy && wx && ix && oh > 0 && ow > 0 && oh <= S && ow <= S && Ty > 0 && Tx > 0,
                "sst_gather_crops: bad LR arguments");
  const int nband = lr ? oh : (S + 3) / 4;                       // gt only: bands of about four rows
  const int W3p = (3 * S + 15) & ~15;
  int P = (3 * span + 3) & ~3;                                   // pitch of a transposed sample's LDS rows: whole dwords, an odd number
  if (((P >> 2) & 1) == 0) P += 4;
  const int64_t stage = (int64_t)span * W3p > (int64_t)S * P ? (int64_t)span * W3p : (int64_t)S * P;
  const int64_t lds = 256 * 4 + (int64_t)W3p * 4 + stage;
  SST_REQUIRE(lds <= 64 * 1024, "sst_gather_crops: %lld B of LDS needed (S %d, span %d) > 64 KiB", (long long)lds, S, span);
  gather_crops_kernel<<<dim3(nband, B), CROPS_NT, (size_t)lds, sst_stream(stream)>>>(arena, arena_bytes, table, N, desc, S, nband, lut,
                                                                                     gt, lr, wy, iy, wx, ix, oh, ow, Ty, Tx, span, P);
  SST_LAUNCH_CHECK("gather_crops_kernel");
  return SST_OK;
}

SST_API int sst_gather_crops_degraded(const uint8_t* arena, int64_t arena_bytes, const int64_t* table, int64_t N, const int* desc,
                                      int B, int S, const float* lut, float* gt, float* lr, const float* wy, const int* iy,
                                      const float* wx, const int* ix, int oh, int ow, int Ty, int Tx, int span, const int* dg, int K,
                                      int quantise, void* stream) {
  SST_REQUIRE(arena && table && desc && lut && lr && dg && arena_bytes > 0 && N > 0 && B > 0 && S > 0,
              "sst_gather_crops_degraded: bad argument (lr and deg are not optional)");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(arena) & 15) == 0 && arena_bytes % 16 == 0,
              "sst_gather_crops_degraded: the arena and its size (%lld B) must be multiples of 16 bytes", (long long)arena_bytes);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(desc) & 15) == 0, "sst_gather_crops_degraded: desc must be 16-byte aligned");
  SST_REQUIRE((reinterpret_cast<uintptr_t>(dg) & 31) == 0, "sst_gather_crops_degraded: deg must be 32-byte aligned (rows of 8 int32)");
  SST_REQUIRE(B <= 65535, "sst_gather_crops_degraded: batch %d > 65535", B);
  SST_REQUIRE(S % 4 == 0 && S <= 16384, "sst_gather_crops_degraded: crop side %d must be a multiple of 4 (and at most 16384)", S);
  SST_REQUIRE(K >= deg::K_MIN && K <= deg::K_MAX && (K & 1), "sst_gather_crops_degraded: the blur window K = %d must be odd and in %d..%d",
              K, deg::K_MIN, deg::K_MAX);
  SST_REQUIRE(K / 2 < S, "sst_gather_crops_degraded: the half window %d (K = %d) must be smaller than the crop side %d", K / 2, K, S);
  SST_REQUIRE(span > 0 && span <= S, "sst_gather_crops_degraded: span %d outside [1, %d]", span, S);
  SST_REQUIRE(wy && iy && wx && ix && oh > 0 && ow > 0 && oh <= S && ow <= S && Ty > 0 && Tx > 0,
              "sst_gather_crops_degraded: bad LR arguments");
  // the band height: the most LR rows (at most deg::ROWS_MAX) whose workgroup fits the LDS budget.  Taps of consecutive LR rows move
  // by the scale, which is at most S / oh.
  const int W3p = (3 * S + 15) & ~15, p = K / 2;
  int R = oh < deg::ROWS_MAX ? oh : deg::ROWS_MAX, nr_max = 0, nline_max = 0, P = 0;
  int64_t lds = 0;
  for (; R >= 1; --R) {
    nr_max = (int)std::min<int64_t>(S, span + (int64_t)(R - 1) * (S / oh));
    nline_max = std::min(S, nr_max + 2 * p);
    P = (3 * nline_max + 3) & ~3;                                // pitch of a transposed sample's LDS rows: whole dwords, an odd number
    if (((P >> 2) & 1) == 0) P += 4;
    lds = deg::Layout(K, R, nr_max, S, std::max<int64_t>((int64_t)nline_max * W3p, (int64_t)S * P), 256 * 4).bytes;
    if (lds <= deg::LDS_BUDGET) break;
  }
  SST_REQUIRE(R >= 1, "sst_gather_crops_degraded: %lld B of LDS needed (S %d, span %d, K %d) > 64 KiB", (long long)lds, S, span, K);
  const int nband = (oh + R - 1) / R;
  gather_crops_degraded_kernel<<<dim3(nband * 3, B), deg::NT, (size_t)lds, sst_stream(stream)>>>(
      arena, arena_bytes, table, N, desc, S, lut, gt, lr, wy, iy, wx, ix, oh, ow, Ty, Tx, dg, K, quantise, R, nr_max, nline_max, P);
  SST_LAUNCH_CHECK("gather_crops_degraded_kernel");
  return SST_OK;
}
