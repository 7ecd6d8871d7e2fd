// Pixel helpers shared by the data (data.hip), metrics (metrics.hip) and tile (tiles.hip) kernels.
#pragma once
#include "common.h"

// bytes a .. a+3 of a byte buffer as one little-endian dword; only the first nvalid (1..4) of them have to be bytes of an image.
// The buffer's base and size are multiples of 16 bytes, so an ALIGNED dword that holds a byte of an image lies inside it: the
// value is funnel-shifted from the one or two aligned dwords that hold the valid bytes and nothing outside the buffer is read.
__device__ __forceinline__ uint32_t load_dword_unaligned(const uint8_t* __restrict__ arena, int64_t a, int nvalid) {
  const int sh = (int)(a & 3);
  const uint32_t* p = reinterpret_cast<const uint32_t*>(arena + (a - sh));
  const uint32_t lo = p[0];
  if (sh + nvalid <= 4) return lo >> (8 * sh);
  return (uint32_t)((((uint64_t)p[1] << 32) | lo) >> (8 * sh));
}

// utils.tensor2img's quantisation, q = rint(clamp(x, 0, 1) * 255.f) in fp32, half to even; the clamp is written with comparisons
// that keep NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float quantise(float x) {
  const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  return rintf(c * 255.f);
}

// the uint8 value of a quantised channel; NaN -> 0
__device__ __forceinline__ uint8_t to_u8(float q) { return q == q ? (uint8_t)(int)q : (uint8_t)0; }
