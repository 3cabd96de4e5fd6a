// pair16.h — the device-side definition of the 16-bit activation formats and of the fp16 hi / lo PAIR format.
//
// A 16-bit map holds (T)v, T = bf16 (math_mode 1) or fp16 (math_mode 2).  A pair map (math_mode 3) holds, per value, two fp16 numbers in two
// planes of a pixel's row: with u = v * 2^-e, hi = rn16(u) and lo = rn16(u - hi), so hi + lo carries u to about 2^-22 relative.  e is the
// map's exponent, exps[slot_out] of the launch's G6dRange16 (include/gen6d_hip.h; 0 without one), and every producer records the largest
// bits(|v|) of the UNSCALED values it stored in rec[slot_out].  The host turns that record into the next exponent and decides whether the
// map left the window in which both planes stay normal fp16 numbers (ops.py: PAIR_KEEP, PAIR_LIMIT, pair_exponent).
#pragma once
#include "g6d_common.h"

// element / 8-element vector of a mode's 16-bit type; C16T3: the same with the pair mode mapped to its fp16 planes
template <int MM> struct C16T;
template <> struct C16T<1> { typedef __bf16 T; typedef bf16x8 V; };
template <> struct C16T<2> { typedef _Float16 T; typedef f16x8 V; };
template <int MM> struct C16T3 { typedef typename C16T<MM == 3 ? 2 : MM>::T T; typedef typename C16T<MM == 3 ? 2 : MM>::V V; };

// What the 16-bit kernels (conv16_tap.hip, conv16w.hip, corr16.hip) share: the 32x32x16 MFMA of a mode (pairs: of its fp16 planes), the buffer
// descriptor of their LDS-DMA and buffer loads, and the offset that always lies beyond it (the out-of-range zero fill).
template <int MM>
__device__ __forceinline__ f32x16 c16_mfma(typename C16T3<MM>::V a, typename C16T3<MM>::V b, f32x16 c) {
  if constexpr (MM == 1) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t c16_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
constexpr unsigned C16_OOB = 0x80000000u;

// The per-value rule: record |v| into amax, scale by 2^-eo, split.
template <typename T>
__device__ __forceinline__ void c16_pair_split(float v, int eo, unsigned& amax, T& hi, T& lo) {
  amax = max(amax, g6d_abs_bits(v));
  const float u = ldexpf(v, -eo);
  hi = (T)u; lo = (T)(u - (float)hi);
}

// Eight consecutive channels to the 16 bytes at o.  MM = 1 / 2: converted, one store (eo, amax, plane_bytes unused).  MM = 3: recorded, scaled
// and split; the hi halves at o, the lo halves plane_bytes further on.
template <int MM>
__device__ __forceinline__ void c16_store8(const float (&v)[8], int eo, unsigned& amax, char* o, long plane_bytes) {
  typedef typename C16T3<MM>::T T;
  typedef typename C16T3<MM>::V V8;
  if constexpr (MM == 3) {
    V8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) { T h, l; c16_pair_split(v[e], eo, amax, h, l); hi[e] = h; lo[e] = l; }
    *reinterpret_cast<V8*>(o) = hi;
    *reinterpret_cast<V8*>(o + plane_bytes) = lo;
  } else {
    V8 q;
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = (T)v[e];
    *reinterpret_cast<V8*>(o) = q;
  }
}
