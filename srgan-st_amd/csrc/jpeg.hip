// sst_jpeg: the JPEG stage of the blind-SR degradation - an all-integer baseline codec round trip, in place, on
// an fp32 LR batch [B,3,h,w] that is on the 1/255 grid.  Every step is int32 arithmetic (tests/jpeg_refs.py restates it in numpy and the
// kernel is held to that bit for bit), so a result depends on neither run, graph replay, batch position nor tile geometry.
// Per sample Q = word 6 of its deg row: 0 keeps the sample's bits (the workgroup leaves at once), outside 0..100 makes it NaN, else
//   pixel     p = (int)rintf(255 clamp01(v)); an MCU with a non-finite element comes out NaN in all three channels
//   colour    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,   Cr = (32768 R - 27439 G - 5329 B + ...) >> 16
//   MCU       8 x 8 (444) or 16 x 16 (420: c = (c00 + c01 + c10 + c11 + 2) >> 2); planes edge-replicated to MCU multiples
//   tables    Annex K, libjpeg's quality rule: s = Q < 50 ? 5000 / Q : 200 - 2 Q, q = clamp((base s + 50) / 100, 1, 255)
//   forward   T[u][x] = rint(8192 C[u][x]) (the host, fp64, once); s = plane - 128; a[y][u] = (sum_x T[u][x] s[y][x] + 512) >> 10;
//             F[v][u] = sum_y T[v][y] a[y][u]   (scale 2^16)
//   quantise  n = sign(F) ((|F| + q 32768) / (q 65536)), D = n q
//   inverse   b[y][u] = (sum_v T[v][y] D[v][u] + 512) >> 10; r[y][x] = (sum_u T[u][x] b[y][u] + 32768) >> 16; clamp(r + 128, 0, 255)
//   back      420 chroma replicated 2 x 2; R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
//             B = Y + ((116130 Cb' + 32768) >> 16), each clamped to 0..255; out = (float)p / 255.f
//
// One 256-thread workgroup per (sample, tile of 32 x 32 pixels = whole MCUs in either mode).  The three planes sit in LDS as int32,
// pitch 33; a thread loads one 2 x 2 quad (colour conversion, edge replication and the 420 average resolved on load).  One wavefront
// per 8 x 8 block and 1-D pass: lane (r, c) makes one element with 8 v_mad_i32_i24 (every operand is below 2^23 in magnitude: |T| <=
// 4096, |a| <= 2897, |D| <= 1152, |b| <= 36000) from a per-wave 8 x 9 LDS buffer; its four rows / columns of T live in 32 registers.
// Only the blocks that hold a pixel of the image are transformed, four at a time; the loop count is the same in every wave, so the
// barriers between the passes are workgroup barriers.  The division by q 65536 is (X >> 16) / q, done as __umulhi(m, 2^32 / q + 1): exact
// for m < 2^15 and 2 <= q <= 255, because the multiplier's excess e = M q - 2^32 <= q gives m e < 2^32.  A workgroup writes only
// its own tile's pixels, after it has read them: in place is safe.  No atomics, no scratch.
#include "common.h"
#include <cmath>

namespace {

constexpr int NT = 256, TILE = 32, PITCH = TILE + 1, BPITCH = 9;

// Annex K.1 / K.2, row-major: row = vertical frequency v, column = horizontal frequency u
const int BASE_TABLES[128] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99,  99,  99,  99,  18, 21, 26, 66, 99,  99,  99,  99,  24, 26, 56, 99, 99,  99,  99,  99,  47, 66, 99, 99, 99,  99,  99,  99,
    99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99};

__host__ __device__ inline int quant_entry(int base, int Q) {
  const int s = Q < 50 ? 5000 / Q : 200 - 2 * Q, q = (base * s + 50) / 100;
  return q < 1 ? 1 : (q > 255 ? 255 : q);
}

struct Consts {
  int T[64];            // T[u][x] = rint(8192 C[u][x])
  int base[128];        // BASE_TABLES
};

const Consts& consts() {
  static const Consts c = [] {
    Consts k;
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; ++u)
      for (int x = 0; x < 8; ++x)
        k.T[u * 8 + x] = (int)std::rint(8192.0 * (u == 0 ? std::sqrt(0.125) : 0.5 * std::cos((2 * x + 1) * u * pi / 16.0)));
    for (int i = 0; i < 128; ++i) k.base[i] = BASE_TABLES[i];
    return k;
  }();
  return c;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(NT) void jpeg_kernel(float* __restrict__ lr, const int* __restrict__ deg, int h, int w, int chroma, int ntx,
                                                  const Consts k) {
  __shared__ int s_plane[3][TILE * PITCH];
  __shared__ int s_buf[2][NT / 64][8 * BPITCH];
  __shared__ int s_T[64], s_q[128], s_bad[16];
  __shared__ unsigned s_m[128];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int Q = deg[b * 8 + 6];
  if (Q == 0) return;                                           // the sample keeps its bits (uniform in the workgroup)
  const int y0 = (blockIdx.x / ntx) * TILE, x0 = (blockIdx.x % ntx) * TILE;
  float* img = lr + (int64_t)b * 3 * h * w;
  const int64_t hw = (int64_t)h * w;
  const int qy = (tid >> 4) * 2, qx = (tid & 15) * 2;           // this thread's 2 x 2 quad of the tile, on load and on store
  if (Q < 0 || Q > 100) {
    for (int i = 0; i < 4; ++i) {
      const int y = y0 + qy + (i >> 1), x = x0 + qx + (i & 1);
      if (y < h && x < w)
        for (int c = 0; c < 3; ++c) img[c * hw + (int64_t)y * w + x] = __int_as_float(0x7fc00000);
    }
    return;
  }
  // ---- constants: T, the sample's two tables and their reciprocal multipliers
  if (tid < 64) s_T[tid] = k.T[tid];
  if (tid < 128) {
    const int q = quant_entry(k.base[tid], Q);
    s_q[tid] = q;
    s_m[tid] = q >= 2 ? 0xffffffffu / (unsigned)q + 1u : 0u;
  }
  if (tid < 16) s_bad[tid] = 0;
  __syncthreads();
  // ---- load: pixel -> integer -> YCbCr, edge replication by clamping the coordinates; the MCU of a non-finite element is marked
  const int mshift = chroma ? 4 : 3, mpr = TILE >> mshift;       // MCUs per tile row
  {
    int cb[4], cr[4];
    for (int i = 0; i < 4; ++i) {
      const int ly = qy + (i >> 1), lx = qx + (i & 1);
      const int64_t at = (int64_t)min(y0 + ly, h - 1) * w + min(x0 + lx, w - 1);
      int p[3];
      bool finite = true;
      for (int c = 0; c < 3; ++c) {
        float v = img[c * hw + at];
        finite = finite && fabsf(v) <= 3.402823466e38f;           // false for NaN and +-inf
        v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        p[c] = finite ? (int)rintf(255.f * v) : 0;
      }
      if (!finite) s_bad[(ly >> mshift) * mpr + (lx >> mshift)] = 1;        // (every writer stores the same value)
      s_plane[0][ly * PITCH + lx] = (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16;
      cb[i] = (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16;
      cr[i] = (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16;
      if (!chroma) s_plane[1][ly * PITCH + lx] = cb[i], s_plane[2][ly * PITCH + lx] = cr[i];
    }
    if (chroma) {
      s_plane[1][(qy >> 1) * PITCH + (qx >> 1)] = (cb[0] + cb[1] + cb[2] + cb[3] + 2) >> 2;
      s_plane[2][(qy >> 1) * PITCH + (qx >> 1)] = (cr[0] + cr[1] + cr[2] + cr[3] + 2) >> 2;
    }
  }
  // ---- this lane's rows and columns of T
  const int wave = tid >> 6, lane = tid & 63, r = lane >> 3, c = lane & 7;
  int t_c[8], t_r[8], tt_r[8], tt_c[8];                           // T[c][i], T[r][i], T[i][r], T[i][c]
#pragma unroll
  for (int i = 0; i < 8; ++i) t_c[i] = s_T[c * 8 + i], t_r[i] = s_T[r * 8 + i], tt_r[i] = s_T[i * 8 + r], tt_c[i] = s_T[i * 8 + c];
  // ---- the blocks that hold a pixel of the image (the MCU grid's, so a partial MCU is transformed whole)
  const int my = min(TILE, ((h - y0 + (1 << mshift) - 1) >> mshift) << mshift), mx = min(TILE, ((w - x0 + (1 << mshift) - 1) >> mshift) << mshift);
  const int nby = my >> 3, nbx = mx >> 3;                         // luma blocks down and across
  const int cby = chroma ? nby >> 1 : nby, cbx = chroma ? nbx >> 1 : nbx;
  const int n_luma = nby * nbx, n_all = n_luma + 2 * cby * cbx;
  int* buf_a = s_buf[0][wave];
  int* buf_b = s_buf[1][wave];
  __syncthreads();
  for (int k0 = 0; k0 < n_all; k0 += NT / 64) {
    const int blk = k0 + wave;
    const bool on = blk < n_all;                                  // (uniform in the wave)
    int pl = 0, by = 0, bx = 0;
    if (on) {
      int j = blk;
      if (j >= n_luma) j -= n_luma, pl = 1 + j / (cby * cbx), j %= cby * cbx, by = j / cbx, bx = j % cbx;
      else by = j / nbx, bx = j % nbx;
    }
    int* plane = s_plane[pl] + by * 8 * PITCH + bx * 8;
    const int* tq = s_q + (pl ? 64 : 0);
    const unsigned* tm = s_m + (pl ? 64 : 0);
    int acc = 0;
    // a[y = r][u = c] = (sum_x T[c][x] s[r][x] + 512) >> 10
    if (on) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += __mul24(t_c[i], plane[r * PITCH + i] - 128);
      buf_a[r * BPITCH + c] = (acc + 512) >> 10;
    }
    __syncthreads();
    // F[v = r][u = c] = sum_y T[r][y] a[y][c], then n = sign(F) ((|F| + q 32768) / (q 65536)), D = n q
    if (on) {
      acc = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += __mul24(t_r[i], buf_a[i * BPITCH + c]);
      const int q = tq[lane];
      const unsigned m = (unsigned)((acc < 0 ? -acc : acc) + q * 32768) >> 16;
      const int n = q == 1 ? (int)m : (int)__umulhi(m, tm[lane]);
      buf_b[r * BPITCH + c] = __mul24(acc < 0 ? -n : n, q);
    }
    __syncthreads();
    // b[y = r][u = c] = (sum_v T[v][r] D[v][c] + 512) >> 10
    if (on) {
      acc = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += __mul24(tt_r[i], buf_b[i * BPITCH + c]);
      buf_a[r * BPITCH + c] = (acc + 512) >> 10;
    }
    __syncthreads();
    // r[y = r][x = c] = (sum_u T[u][c] b[r][u] + 32768) >> 16, back into the plane
    if (on) {
      acc = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += __mul24(tt_c[i], buf_a[r * BPITCH + i]);
      plane[r * PITCH + c] = clamp255(((acc + 32768) >> 16) + 128);
    }
    __syncthreads();
  }
  // ---- store: the quad's pixels inside the image
  for (int i = 0; i < 4; ++i) {
    const int ly = qy + (i >> 1), lx = qx + (i & 1), y = y0 + ly, x = x0 + lx;
    if (y >= h || x >= w) continue;
    const int64_t at = (int64_t)y * w + x;
    if (s_bad[(ly >> mshift) * mpr + (lx >> mshift)]) {
      for (int ch = 0; ch < 3; ++ch) img[ch * hw + at] = __int_as_float(0x7fc00000);
      continue;
    }
    const int cat = chroma ? (ly >> 1) * PITCH + (lx >> 1) : ly * PITCH + lx;
    const int Y = s_plane[0][ly * PITCH + lx], cb = s_plane[1][cat] - 128, cr = s_plane[2][cat] - 128;
    img[at] = (float)clamp255(Y + ((91881 * cr + 32768) >> 16)) / 255.f;
    img[hw + at] = (float)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)) / 255.f;
    img[2 * hw + at] = (float)clamp255(Y + ((116130 * cb + 32768) >> 16)) / 255.f;
  }
}

}  // namespace

SST_API int sst_jpeg_tables(int quality, int* out128) {
  SST_REQUIRE(out128, "sst_jpeg_tables: null pointer");
  SST_REQUIRE(quality >= 1 && quality <= 100, "sst_jpeg_tables: quality %d outside 1..100", quality);
  for (int i = 0; i < 128; ++i) out128[i] = quant_entry(BASE_TABLES[i], quality);
  return SST_OK;
}

SST_API int sst_jpeg(float* lr, const int* deg, int B, int h, int w, int chroma, void* stream) {
  SST_REQUIRE(lr && deg, "sst_jpeg: null pointer");
  SST_REQUIRE(B > 0 && B <= 65535, "sst_jpeg: batch %d outside [1, 65535]", B);
  SST_REQUIRE(h > 0 && w > 0 && h <= 8192 && w <= 8192, "sst_jpeg: image %dx%d outside 1..8192", w, h);
  SST_REQUIRE(chroma == 0 || chroma == 1, "sst_jpeg: chroma %d must be 0 (444) or 1 (420)", chroma);
  SST_REQUIRE((reinterpret_cast<uintptr_t>(deg) & 31) == 0, "sst_jpeg: deg must be 32-byte aligned (rows of 8 int32)");
  const int ntx = (w + TILE - 1) / TILE, nty = (h + TILE - 1) / TILE;
  jpeg_kernel<<<dim3((unsigned)(ntx * nty), B), NT, 0, sst_stream(stream)>>>(lr, deg, h, w, chroma, ntx, consts());
  SST_LAUNCH_CHECK("jpeg_kernel");
  return SST_OK;
}
