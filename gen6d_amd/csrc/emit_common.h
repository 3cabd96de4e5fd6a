// What the two annotated-output kernels share (emit.hip: the working-resolution canvas, emit_source.hip: the camera's own frame): the
// tile shape, the exact integer drawing rules of include/gen6d_hip.h (edge and disc tests, the per-tile cull), the forward colour
// formulas and the sink stores.  Everything is __forceinline__ and works on scalar words: a thread's 8 pixels stay in registers.
#pragma once
#include "g6d_common.h"

namespace {

constexpr int TW = 128, TH = 16;
constexpr int QMIN = -8192, QMAX = 16383;      // corner range inside which the 64-bit edge rule is exact (header)

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// pixel centre within thickness / 2 of the segment a-b, th2 = thickness^2 (header: every term < 2^63)
__device__ __forceinline__ bool edge_hit(int x, int y, int ax, int ay, int bx, int by, long long th2) {
  const long long dx = bx - ax, dy = by - ay, px = x - ax, py = y - ay;
  const long long L = dx * dx + dy * dy, pp = px * px + py * py;
  if (L == 0) return 4 * pp <= th2;
  const long long s = px * dx + py * dy, t = min(max(s, 0LL), L);
  return L * pp - 2 * t * s + t * t <= ((th2 * L) >> 2);
}

// 4 consecutive pixels of one row, each R | G << 8 | B << 16 (scalars, not a byte array: the compiler keeps them in registers)
struct Row { unsigned a, b, c, d; };

__device__ __forceinline__ unsigned pixel(const unsigned char* p, bool in) {
  return in ? (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) : 0u;
}
__device__ __forceinline__ void paint(Row& r, unsigned e, unsigned d, unsigned line, unsigned dot) {
  r.a = (e & 1u) ? line : ((d & 1u) ? dot : r.a); r.b = (e & 2u) ? line : ((d & 2u) ? dot : r.b);
  r.c = (e & 4u) ? line : ((d & 4u) ? dot : r.c); r.d = (e & 8u) ? line : ((d & 8u) ? dot : r.d);
}
__device__ __forceinline__ unsigned swap1(unsigned p) { return ((p & 0xffu) << 16) | (p & 0xff00u) | (p >> 16); }
__device__ __forceinline__ void swap_rb(Row& r) { r.a = swap1(r.a); r.b = swap1(r.b); r.c = swap1(r.c); r.d = swap1(r.d); }
__device__ __forceinline__ unsigned luma(unsigned p, int cyr, int cyg, int cyb) {
  return (unsigned)sat8((cyr * (int)(p & 255u) + cyg * (int)((p >> 8) & 255u) + cyb * (int)(p >> 16) + (1 << 19) + (16 << 20)) >> 20);
}
// 4 bytes at o (the first `left` of them when the sink ends inside): one dword where the address allows
__device__ __forceinline__ void put4(unsigned char* o, unsigned w, bool full, int left) {
  if (full && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) { *reinterpret_cast<unsigned*>(o) = w; return; }
  if (left > 0) o[0] = (unsigned char)w;
  if (left > 1) o[1] = (unsigned char)(w >> 8);
  if (left > 2) o[2] = (unsigned char)(w >> 16);
  if (left > 3) o[3] = (unsigned char)(w >> 24);
}
// 4 packed 3-byte pixels (12 bytes; the first `left` bytes when the sink ends inside)
__device__ __forceinline__ void put12(unsigned char* o, const Row& r, bool full, int left) {
  const unsigned w0 = r.a | (r.b << 24), w1 = (r.b >> 8) | (r.c << 16), w2 = (r.c >> 16) | (r.d << 8);
  if (full && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
    unsigned* o32 = reinterpret_cast<unsigned*>(o);
    o32[0] = w0; o32[1] = w1; o32[2] = w2;
    return;
  }
  put4(o, w0, false, left); put4(o + 4, w1, false, left - 4); put4(o + 8, w2, false, left - 8);
}
// 4 packed 4-byte pixels with alpha 255 (the first `left` pixels when the sink ends inside)
__device__ __forceinline__ void put16(unsigned char* o, const Row& r, bool full, int left) {
  const unsigned w0 = r.a | 0xff000000u, w1 = r.b | 0xff000000u, w2 = r.c | 0xff000000u, w3 = r.d | 0xff000000u;
  const uintptr_t al = reinterpret_cast<uintptr_t>(o);
  if (full && (al & 15u) == 0) { *reinterpret_cast<uint4*>(o) = make_uint4(w0, w1, w2, w3); return; }
  const bool dw = (al & 3u) == 0;
  if (left > 0) put4(o, w0, dw, 4);
  if (left > 1) put4(o + 4, w1, dw, 4);
  if (left > 2) put4(o + 8, w2, dw, 4);
  if (left > 3) put4(o + 12, w3, dw, 4);
}

// Wave 0 (t < 64) of a block: the primitives of the box q that can touch the tile at (X0, Y0) of a pw x ph picture -> sp (edges
// (ax, ay, bx, by) first, then discs (qx, qy, -, -)) and sn = (listed edges, listed primitives).  Bounding boxes grown by the half
// thickness / radius, and the edge's supporting line against the rectangle's corners; a corner outside [QMIN, QMAX] empties the list.
__device__ __forceinline__ void cull_tile(int (*sp)[4], int* sn, int t, bool draw, const int* __restrict__ q, int th, long long th2, int rad,
                                          int X0, int Y0, int pw, int ph) {
  bool hit = false;
  int ax = 0, ay = 0, bx = 0, by = 0;
  const bool bad = draw && t < 8 && (q[2 * t] < QMIN || q[2 * t] > QMAX || q[2 * t + 1] < QMIN || q[2 * t + 1] > QMAX);
  if (draw && t < 20 && X0 < pw && Y0 < ph) {
    const int x1 = min(X0 + TW, pw) - 1, y1 = min(Y0 + TH, ph) - 1;     // pixel rectangle [X0, x1] x [Y0, y1] inside the picture
    if (t < 12) {
      const int a = t < 4 ? t : (t < 8 ? t : t - 8), b = t < 4 ? ((t + 1) & 3) : (t < 8 ? 4 + ((t + 1) & 3) : t - 4);
      ax = q[2 * a]; ay = q[2 * a + 1]; bx = q[2 * b]; by = q[2 * b + 1];
      const int hw = (th + 1) >> 1;
      hit = th > 0 && max(ax, bx) + hw >= X0 && min(ax, bx) - hw <= x1 && max(ay, by) + hw >= Y0 && min(ay, by) - hw <= y1;
      const long long dx = bx - ax, dy = by - ay, L = dx * dx + dy * dy;
      if (hit && L > 0) {
        // the supporting line: cross(d, c - a) is linear in c, so if it has one sign at the rectangle's four corners, every pixel's
        // |cross| is at least the smallest corner value, and a pixel is covered only if cross^2 <= thickness^2 L / 4
        const long long c00 = dx * (Y0 - ay) - dy * (X0 - ax), c01 = dx * (Y0 - ay) - dy * (x1 - ax);
        const long long c10 = dx * (y1 - ay) - dy * (X0 - ax), c11 = dx * (y1 - ay) - dy * (x1 - ax);
        const long long lo = min(min(c00, c01), min(c10, c11)), hi = max(max(c00, c01), max(c10, c11));
        const long long m = lo > 0 ? lo : (hi < 0 ? -hi : 0);
        if (m * m > ((th2 * L) >> 2)) hit = false;
      }
    } else {
      ax = q[2 * (t - 12)]; ay = q[2 * (t - 12) + 1];
      hit = rad >= 0 && ax + rad >= X0 && ax - rad <= x1 && ay + rad >= Y0 && ay - rad <= y1;
    }
  }
  if (__ballot(bad)) hit = false;
  const unsigned long long m = __ballot(hit);
  if (hit) {
    const int pos = __popcll(m & ((1ull << t) - 1));
    sp[pos][0] = ax; sp[pos][1] = ay; sp[pos][2] = bx; sp[pos][3] = by;
  }
  if (t == 0) { sn[0] = __popcll(m & 0xfffull); sn[1] = __popcll(m); }
}

// The listed primitives against a thread's pixels (X .. X+3, Y) and (X .. X+3, Y+1): bit i of a mask = pixel X + i; e: edges, d: discs
__device__ __forceinline__ void cover(const int (*sp)[4], int ne, int n, int X, int Y, long long th2, int rad2, unsigned& e0, unsigned& e1,
                                      unsigned& d0, unsigned& d1) {
  for (int l = 0; l < ne; ++l) {
    const int ax = sp[l][0], ay = sp[l][1], bx = sp[l][2], by = sp[l][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      e0 |= (edge_hit(X + i, Y, ax, ay, bx, by, th2) ? 1u : 0u) << i;
      e1 |= (edge_hit(X + i, Y + 1, ax, ay, bx, by, th2) ? 1u : 0u) << i;
    }
  }
  for (int l = ne; l < n; ++l) {
    const int ux = X - sp[l][0], uy = Y - sp[l][1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d0 |= ((ux + i) * (ux + i) + uy * uy <= rad2 ? 1u : 0u) << i;
      d1 |= ((ux + i) * (ux + i) + (uy + 1) * (uy + 1) <= rad2 ? 1u : 0u) << i;
    }
  }
}

// round(k * 2^20) of a limited-range forward matrix (header)
struct Fwd { int cyr, cyg, cyb, cbr, cbg, cbb, crr, crg, crb; };
__device__ __forceinline__ Fwd forward_matrix(bool m709) {
  return Fwd{m709 ? 191455 : 269262, m709 ? 644067 : 528618, m709 ? 65019 : 102662,
             m709 ? -105533 : -155423, m709 ? -355018 : -305128, 460551,
             460551, m709 ? -418321 : -385654, m709 ? -42230 : -74897};
}
// the 4 Y bytes of a row
__device__ __forceinline__ unsigned luma4(const Row& r, const Fwd& m) {
  return luma(r.a, m.cyr, m.cyg, m.cyb) | (luma(r.b, m.cyr, m.cyg, m.cyb) << 8) | (luma(r.c, m.cyr, m.cyg, m.cyb) << 16) |
         (luma(r.d, m.cyr, m.cyg, m.cyb) << 24);
}
// the 2 UV pairs of two rows: channel sums of a 2 x 2 block, R | G << 8 | B << 16 of four pixels summed in 16-bit fields
__device__ __forceinline__ unsigned chroma4(const Row& r0, const Row& r1, const Fwd& m) {
  const unsigned lo0 = (r0.a & 0xff00ffu) + (r0.b & 0xff00ffu) + (r1.a & 0xff00ffu) + (r1.b & 0xff00ffu);
  const unsigned g0 = ((r0.a >> 8) & 255u) + ((r0.b >> 8) & 255u) + ((r1.a >> 8) & 255u) + ((r1.b >> 8) & 255u);
  const unsigned lo1 = (r0.c & 0xff00ffu) + (r0.d & 0xff00ffu) + (r1.c & 0xff00ffu) + (r1.d & 0xff00ffu);
  const unsigned g1 = ((r0.c >> 8) & 255u) + ((r0.d >> 8) & 255u) + ((r1.c >> 8) & 255u) + ((r1.d >> 8) & 255u);
  const int sr0 = lo0 & 0xffff, sb0 = lo0 >> 16, sr1 = lo1 & 0xffff, sb1 = lo1 >> 16;
  return (unsigned)sat8((m.cbr * sr0 + m.cbg * (int)g0 + m.cbb * sb0 + (1 << 21) + (128 << 22)) >> 22) |
         ((unsigned)sat8((m.crr * sr0 + m.crg * (int)g0 + m.crb * sb0 + (1 << 21) + (128 << 22)) >> 22) << 8) |
         ((unsigned)sat8((m.cbr * sr1 + m.cbg * (int)g1 + m.cbb * sb1 + (1 << 21) + (128 << 22)) >> 22) << 16) |
         ((unsigned)sat8((m.crr * sr1 + m.crg * (int)g1 + m.crb * sb1 + (1 << 21) + (128 << 22)) >> 22) << 24);
}

// A thread's annotated RGB rows (X .. X+3, Y) and (X .. X+3, Y+1) -> the sink, in its format.  (frame_emit_kernel keeps this tail written
// out in its body: calling it from there changed that kernel's measured register figures.)
__device__ __forceinline__ void store_rows(const G6dSink& k, Row r0, Row r1, int X, int Y, const Fwd& m) {
  const int fmt = k.format, sw = k.width, sh = k.height;
  const bool full = X + 4 <= sw;
  unsigned char* const p0 = static_cast<unsigned char*>(k.plane0);
  if (fmt == G6D_FMT_NV12) {                               // (block-uniform)
    put4(p0 + (size_t)Y * k.pitch0 + X, luma4(r0, m), full, sw - X);
    if (Y + 1 < sh) {
      put4(p0 + (size_t)(Y + 1) * k.pitch0 + X, luma4(r1, m), full, sw - X);
      // (an even width: a chroma pair is inside whole or not at all)
      put4(static_cast<unsigned char*>(k.plane1) + (size_t)(Y >> 1) * k.pitch1 + X, chroma4(r0, r1, m), full, sw - X);
    }
  } else {
    if (fmt == G6D_FMT_BGR24 || fmt == G6D_FMT_BGRA32) { swap_rb(r0); swap_rb(r1); }
    if (fmt == G6D_FMT_RGB24 || fmt == G6D_FMT_BGR24) {
      put12(p0 + (size_t)Y * k.pitch0 + (size_t)X * 3, r0, full, 3 * (sw - X));
      if (Y + 1 < sh) put12(p0 + (size_t)(Y + 1) * k.pitch0 + (size_t)X * 3, r1, full, 3 * (sw - X));
    } else {                                               // RGBA32 / BGRA32, alpha 255
      put16(p0 + (size_t)Y * k.pitch0 + (size_t)X * 4, r0, full, sw - X);
      if (Y + 1 < sh) put16(p0 + (size_t)(Y + 1) * k.pitch0 + (size_t)X * 4, r1, full, sw - X);
    }
  }
}

// ---- sinks of the formats after NV12 and of the full-range matrices (header) ----
// Both kernels send such a sink here on a block-uniform test and keep the code above, as it was measured, for everything else.
__device__ __forceinline__ bool extended_sink(const G6dSink& k) { return k.format > G6D_FMT_NV12 || (k.format == G6D_FMT_NV12 && k.matrix > 1); }
// sat8(v >> sh) clamped BEFORE the shift: the form emit_source.hip needs (see sat8s20 there), used for every conversion below
__device__ __forceinline__ unsigned satsh(int v, int sh) { return (unsigned)(min(max(v, 0), (256 << sh) - 1) >> sh); }

// a forward matrix and the constant of its Y row: 2^19 + 16 2^20 limited range, 2^19 full range
struct FwdX { Fwd m; int yadd; };
__device__ __forceinline__ FwdX forward_matrix_x(int matrix) {
  if (matrix < 2) return FwdX{forward_matrix(matrix == 1), (1 << 19) + (16 << 20)};
  const bool m709 = (matrix & 1) != 0;
  return FwdX{Fwd{m709 ? 222927 : 313524, m709 ? 749942 : 615514, m709 ? 75707 : 119538,
                  m709 ? -120138 : -176932, m709 ? -404150 : -347356, 524288,
                  524288, m709 ? -476214 : -439026, m709 ? -48074 : -85262}, 1 << 19};
}
__device__ __forceinline__ unsigned luma_x(unsigned p, const FwdX& f) {
  return satsh(f.m.cyr * (int)(p & 255u) + f.m.cyg * (int)((p >> 8) & 255u) + f.m.cyb * (int)(p >> 16) + f.yadd, 20);
}
__device__ __forceinline__ unsigned luma4_x(const Row& r, const FwdX& f) {
  return luma_x(r.a, f) | (luma_x(r.b, f) << 8) | (luma_x(r.c, f) << 16) | (luma_x(r.d, f) << 24);
}
// Cb | Cr << 8 of one chroma block from its channel sums (rb = sR | sB << 16, g = sG); sh = 20 + log2(pixels of the block)
__device__ __forceinline__ unsigned chroma_x(unsigned rb, unsigned g, const Fwd& m, int sh) {
  const int sr = rb & 0xffff, sb = rb >> 16, add = (1 << (sh - 1)) + (128 << sh);
  return satsh(m.cbr * sr + m.cbg * (int)g + m.cbb * sb + add, sh) | (satsh(m.crr * sr + m.crg * (int)g + m.crb * sb + add, sh) << 8);
}
// the chroma of a thread's pixels as U0 V0 U1 V1: of the two 2 x 2 blocks of two rows (4:2:0), of the two pairs of one row (4:2:2)
__device__ __forceinline__ unsigned chroma420_x(const Row& r0, const Row& r1, const Fwd& m) {
  const unsigned lo0 = (r0.a & 0xff00ffu) + (r0.b & 0xff00ffu) + (r1.a & 0xff00ffu) + (r1.b & 0xff00ffu);
  const unsigned g0 = ((r0.a >> 8) & 255u) + ((r0.b >> 8) & 255u) + ((r1.a >> 8) & 255u) + ((r1.b >> 8) & 255u);
  const unsigned lo1 = (r0.c & 0xff00ffu) + (r0.d & 0xff00ffu) + (r1.c & 0xff00ffu) + (r1.d & 0xff00ffu);
  const unsigned g1 = ((r0.c >> 8) & 255u) + ((r0.d >> 8) & 255u) + ((r1.c >> 8) & 255u) + ((r1.d >> 8) & 255u);
  return chroma_x(lo0, g0, m, 22) | (chroma_x(lo1, g1, m, 22) << 16);
}
__device__ __forceinline__ unsigned chroma422_x(const Row& r, const Fwd& m) {
  return chroma_x((r.a & 0xff00ffu) + (r.b & 0xff00ffu), ((r.a >> 8) & 255u) + ((r.b >> 8) & 255u), m, 21) |
         (chroma_x((r.c & 0xff00ffu) + (r.d & 0xff00ffu), ((r.c >> 8) & 255u) + ((r.d >> 8) & 255u), m, 21) << 16);
}

// neighbouring bytes swapped: Y0 U Y1 V <-> U Y0 V Y1
__device__ __forceinline__ unsigned swap_bytes(unsigned w) { return ((w >> 8) & 0x00ff00ffu) | ((w << 8) & 0xff00ff00u); }
// 2 bytes at o (the first `left` of them): one 16-bit store where the address allows
__device__ __forceinline__ void put2(unsigned char* o, unsigned w, int left) {
  if (left > 1 && (reinterpret_cast<uintptr_t>(o) & 1u) == 0) { *reinterpret_cast<unsigned short*>(o) = (unsigned short)w; return; }
  if (left > 0) o[0] = (unsigned char)w;
  if (left > 1) o[1] = (unsigned char)(w >> 8);
}
// A thread's 8-bit YUV samples -> a YUV sink in its layout: y0 / y1 the 4 Y bytes of rows Y / Y + 1, c0 / c1 the chroma U0 V0 U1 V1 of
// those rows (4:2:0 sinks take c0: one block row).  Even widths: a pair of pixels is inside the sink whole or not at all.
__device__ __forceinline__ void store_yuv8(const G6dSink& k, int X, int Y, unsigned y0, unsigned y1, unsigned c0, unsigned c1) {
  const int fmt = k.format, sw = k.width, sh = k.height;
  const bool full = X + 4 <= sw, two = Y + 1 < sh;
  unsigned char* const p0 = static_cast<unsigned char*>(k.plane0);
  unsigned char* const p1 = static_cast<unsigned char*>(k.plane1);
  if (fmt > G6D_FMT_YV12) return;                          // P010 and GRAY8 are read-only formats: nothing is written
  if (fmt == G6D_FMT_YUYV422 || fmt == G6D_FMT_UYVY422) {  // (block-uniform, as every format test here)
    const bool uyvy = fmt == G6D_FMT_UYVY422;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j == 1 && !two) break;
      const unsigned y = j ? y1 : y0, c = j ? c1 : c0;
      unsigned w0 = (y & 255u) | ((c & 255u) << 8) | (((y >> 8) & 255u) << 16) | (((c >> 8) & 255u) << 24);
      unsigned w1 = ((y >> 16) & 255u) | (((c >> 16) & 255u) << 8) | ((y >> 24) << 16) | ((c >> 24) << 24);
      if (uyvy) { w0 = swap_bytes(w0); w1 = swap_bytes(w1); }
      unsigned char* o = p0 + (size_t)(Y + j) * k.pitch0 + (size_t)X * 2;
      put4(o, w0, true, 4);
      if (full) put4(o + 4, w1, true, 4);
    }
    return;
  }
  put4(p0 + (size_t)Y * k.pitch0 + X, y0, full, sw - X);
  if (!two) return;
  put4(p0 + (size_t)(Y + 1) * k.pitch0 + X, y1, full, sw - X);
  if (fmt == G6D_FMT_NV12) { put4(p1 + (size_t)(Y >> 1) * k.pitch1 + X, c0, full, sw - X); return; }
  unsigned char* const second = p1 + (size_t)k.pitch1 * (sh >> 1);
  const size_t o = (size_t)(Y >> 1) * k.pitch1 + (X >> 1);
  put2((fmt == G6D_FMT_I420 ? p1 : second) + o, (c0 & 255u) | (((c0 >> 16) & 255u) << 8), full ? 2 : 1);
  put2((fmt == G6D_FMT_I420 ? second : p1) + o, ((c0 >> 8) & 255u) | ((c0 >> 24) << 8), full ? 2 : 1);
}
// A thread's annotated RGB rows -> an extended sink (store_rows' counterpart)
__device__ __forceinline__ void store_rows_x(const G6dSink& k, const Row& r0, const Row& r1, int X, int Y, const FwdX& f) {
  const bool c422 = k.format == G6D_FMT_YUYV422 || k.format == G6D_FMT_UYVY422;
  const unsigned c0 = c422 ? chroma422_x(r0, f.m) : chroma420_x(r0, r1, f.m);
  store_yuv8(k, X, Y, luma4_x(r0, f), luma4_x(r1, f), c0, c422 ? chroma422_x(r1, f.m) : c0);
}

}  // namespace
