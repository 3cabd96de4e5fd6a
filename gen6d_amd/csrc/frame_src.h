// One tap of a camera-native frame (G6dFrame, include/gen6d_hip.h) -> RGB by the ingest's tap rules: packed formats through `ro`, `bpp` and
// the row pitch, NV12 through the header's integer conversion with chroma UV[y>>1][x>>1].  Shared by the kernels that read source pictures
// (ingest.hip, frame_crop.hip).  The formats after NV12 and the full-range matrices follow below on a description of their own (`Yuv`).
#pragma once
#include "g6d_common.h"

namespace {

struct Src {
  const unsigned char* p0; const unsigned char* p1;
  int pitch0, pitch1, bpp, ro, nv12;
  int cvr, cug, cvg, cub;
};

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// NV12: the chroma terms of one UV sample (shared by the up to four luma taps of its 2 x 2 block), then one luma tap -> RGB
// (TWINS: yuv_chroma<int> / yuv_tap<int> below are the same formula for every 8-bit layout and either range; a change of the rule goes
// into both.  tests/test_pixel_formats_cpu.py / _gpu.py hold them together: i420 / yv12 / p010 frames against nv12 frames of the same samples)
struct Chroma { int r, g, b; };
__device__ __forceinline__ Chroma chroma(const Src& s, int cx, int cy) {
  const unsigned char* uv = s.p1 + (size_t)cy * s.pitch1 + 2 * cx;
  const int d = (int)uv[0] - 128, e = (int)uv[1] - 128;
  return Chroma{s.cvr * e + (1 << 19), -s.cug * d - s.cvg * e + (1 << 19), s.cub * d + (1 << 19)};
}
__device__ __forceinline__ void tap_nv12(const Src& s, const Chroma& k, int x, int y, int& r, int& g, int& b) {
  const int c = max((int)s.p0[(size_t)y * s.pitch0 + x] - 16, 0) * 1220542;
  r = sat8((c + k.r) >> 20); g = sat8((c + k.g) >> 20); b = sat8((c + k.b) >> 20);
}
__device__ __forceinline__ void tap_packed(const Src& s, int x, int y, int& r, int& g, int& b) {
  const unsigned char* p = s.p0 + (size_t)y * s.pitch0 + (size_t)x * s.bpp;
  r = p[s.ro]; g = p[1]; b = p[2 - s.ro];
}

__device__ __forceinline__ Src source_of(const G6dFrame& f) {
  Src s;
  s.p0 = static_cast<const unsigned char*>(f.plane0); s.p1 = static_cast<const unsigned char*>(f.plane1);
  s.pitch0 = f.pitch0; s.pitch1 = f.pitch1;
  s.nv12 = f.format == G6D_FMT_NV12;
  s.bpp = f.format >= G6D_FMT_RGBA32 ? 4 : 3;
  s.ro = (f.format == G6D_FMT_BGR24 || f.format == G6D_FMT_BGRA32) ? 2 : 0;
  const bool m709 = f.matrix == 1;
  s.cvr = m709 ? 1880097 : 1673527; s.cug = m709 ? 223347 : 409993; s.cvg = m709 ? 558891 : 852492; s.cub = m709 ? 2214593 : 2116026;
  return s;
}

// ---- the formats after NV12 and the full-range matrices ----
// Kernels send a frame here on a block-uniform test (`extended`) and keep the code above, as it was measured, for everything else.  One
// description covers every YUV layout: where a luma sample and the two chroma samples of a pixel lie, and the constants of the
// matrix.  8-bit formats convert in 32-bit (limited range: the bounds of the code above; full range: 2^20 255 + 1858077 128 + 2^19 <
// 2^31), P010 in 64-bit (its limited-range sums pass 2^31, header).
__device__ __forceinline__ bool extended(const G6dFrame& f) { return f.format > G6D_FMT_NV12 || (f.format == G6D_FMT_NV12 && f.matrix > 1); }

struct Yuv {
  const unsigned char *py, *pu, *pv;           // luma sample (0, 0); the U and the V sample of chroma block (0, 0)
  int pitch, cpitch;                           // bytes between luma rows, between chroma rows
  int ystep, cstep, csy;                       // bytes between luma samples of a row, between chroma samples; chroma row = y >> csy
  int kind;                                    // 0: 8-bit YUV, 1: P010, 2: GRAY8
  int cy, yoff, cvr, cug, cvg, cub;            // c = max(Y - yoff, 0) (yoff in the sample's own scale), constants round(k 2^20)
};

__device__ __forceinline__ Yuv yuv_of(const G6dFrame& f) {
  Yuv s;
  const unsigned char* p0 = static_cast<const unsigned char*>(f.plane0);
  const unsigned char* p1 = static_cast<const unsigned char*>(f.plane1);
  const int fmt = f.format;
  s.py = p0; s.pu = p1; s.pv = p1 + 1;         // NV12
  s.pitch = f.pitch0; s.cpitch = f.pitch1; s.ystep = 1; s.cstep = 2; s.csy = 1;
  s.kind = fmt == G6D_FMT_P010 ? 1 : (fmt == G6D_FMT_GRAY8 ? 2 : 0);
  if (fmt == G6D_FMT_YUYV422 || fmt == G6D_FMT_UYVY422) {
    const int o = fmt == G6D_FMT_UYVY422 ? 1 : 0;
    s.py = p0 + o; s.pu = p0 + 1 - o; s.pv = p0 + 3 - o;
    s.cpitch = f.pitch0; s.ystep = 2; s.cstep = 4; s.csy = 0;
  } else if (fmt == G6D_FMT_I420 || fmt == G6D_FMT_YV12) {
    const unsigned char* second = p1 + (size_t)f.pitch1 * (f.height >> 1);
    s.pu = fmt == G6D_FMT_I420 ? p1 : second; s.pv = fmt == G6D_FMT_I420 ? second : p1;
    s.cstep = 1;
  } else if (fmt == G6D_FMT_P010) {
    s.pv = p1 + 2; s.ystep = 2; s.cstep = 4;
  }
  const int m = f.matrix;
  const bool full = m >= 2, m709 = (m & 1) != 0;
  s.cy = full ? (1 << 20) : 1220542;
  s.yoff = full ? 0 : (s.kind == 1 ? 64 : 16);
  if (full) { s.cvr = m709 ? 1651297 : 1470104; s.cug = m709 ? 196424 : 360853; s.cvg = m709 ? 490864 : 748826; s.cub = m709 ? 1945738 : 1858077; }
  else { s.cvr = m709 ? 1880097 : 1673527; s.cug = m709 ? 223347 : 409993; s.cvg = m709 ? 558891 : 852492; s.cub = m709 ? 2214593 : 2116026; }
  return s;
}

// T = int: 8-bit samples, >> 20; T = long long: 16-bit little-endian words holding 10-bit samples (word >> 6), >> 22
// (TWINS of chroma / tap_nv12 above, which stay as measured for NV12 under matrix 0 / 1)
template <typename T> struct Kc { T r, g, b; };
template <typename T> __device__ __forceinline__ int sample(const unsigned char* p) {
  if constexpr (sizeof(T) == 8) return (int)(((unsigned)p[0] | ((unsigned)p[1] << 8)) >> 6);   // (bytes: a plane may start at an odd address)
  else return (int)p[0];
}
template <typename T> __device__ __forceinline__ Kc<T> yuv_chroma(const Yuv& s, int cx, int cy) {
  constexpr int mid = sizeof(T) == 8 ? 512 : 128;
  constexpr T rnd = sizeof(T) == 8 ? (T)1 << 21 : (T)1 << 19;
  const size_t o = (size_t)cy * s.cpitch + (size_t)cx * s.cstep;
  const T d = sample<T>(s.pu + o) - mid, e = sample<T>(s.pv + o) - mid;
  return Kc<T>{s.cvr * e + rnd, -s.cug * d - s.cvg * e + rnd, s.cub * d + rnd};
}
template <typename T> __device__ __forceinline__ void yuv_tap(const Yuv& s, const Kc<T>& k, int x, int y, int& r, int& g, int& b) {
  constexpr int sh = sizeof(T) == 8 ? 22 : 20;
  const T c = (T)max(sample<T>(s.py + (size_t)y * s.pitch + (size_t)x * s.ystep) - s.yoff, 0) * s.cy;
  r = sat8((int)((c + k.r) >> sh)); g = sat8((int)((c + k.g) >> sh)); b = sat8((int)((c + k.b) >> sh));
}

// The four taps (x0 | x1, y0 | y1) of one pixel -> RGB each.  LAZY: the taps whose weight is 0 (wa == 0: the x1 column, wb == 0: the y1
// row) are not loaded and come back as 0; a chroma sample is loaded and converted once for the taps that share it (4:2:0: its 2 x 2
// block, 4:2:2: its pair in a row).
struct Tap { int r, g, b; };
template <typename T, bool LAZY>
__device__ __forceinline__ void yuv_taps(const Yuv& s, int x0, int x1, int y0, int y1, bool wa, bool wb, Tap& t00, Tap& t01, Tap& t10, Tap& t11) {
  const bool sx = (x1 >> 1) == (x0 >> 1), sy = (y1 >> s.csy) == (y0 >> s.csy);
  const Kc<T> k00 = yuv_chroma<T>(s, x0 >> 1, y0 >> s.csy);
  yuv_tap<T>(s, k00, x0, y0, t00.r, t00.g, t00.b);
  Kc<T> k01 = k00;
  t01 = t10 = t11 = Tap{0, 0, 0};
  if (!LAZY || wa) { if (!sx) k01 = yuv_chroma<T>(s, x1 >> 1, y0 >> s.csy); yuv_tap<T>(s, k01, x1, y0, t01.r, t01.g, t01.b); }
  if (!LAZY || wb) {
    const Kc<T> k10 = sy ? k00 : yuv_chroma<T>(s, x0 >> 1, y1 >> s.csy);
    yuv_tap<T>(s, k10, x0, y1, t10.r, t10.g, t10.b);
    if (!LAZY || wa) {
      const Kc<T> k11 = sx ? k10 : (sy ? k01 : yuv_chroma<T>(s, x1 >> 1, y1 >> s.csy));
      yuv_tap<T>(s, k11, x1, y1, t11.r, t11.g, t11.b);
    }
  }
}
__device__ __forceinline__ Tap gray_tap(const Yuv& s, int x, int y) {
  const int v = s.py[(size_t)y * s.pitch + x];
  return Tap{v, v, v};
}
template <bool LAZY>
__device__ __forceinline__ void ext_taps(const Yuv& s, int x0, int x1, int y0, int y1, bool wa, bool wb, Tap& t00, Tap& t01, Tap& t10, Tap& t11) {
  if (s.kind == 0) yuv_taps<int, LAZY>(s, x0, x1, y0, y1, wa, wb, t00, t01, t10, t11);           // (block-uniform)
  else if (s.kind == 1) yuv_taps<long long, LAZY>(s, x0, x1, y0, y1, wa, wb, t00, t01, t10, t11);
  else {
    t00 = gray_tap(s, x0, y0);
    t01 = t10 = t11 = Tap{0, 0, 0};
    if (!LAZY || wa) t01 = gray_tap(s, x1, y0);
    if (!LAZY || wb) t10 = gray_tap(s, x0, y1);
    if (!LAZY || (wa && wb)) t11 = gray_tap(s, x1, y1);
  }
}

}  // namespace
