// Source-view annotated output (gen6d_amd/emit.py, Sink(view="source")): the camera's own frame of a push, as the G6dFrame table of the
// ingest describes it (packed RGB / BGR(A) or NV12, any size, pitch and alignment, not turned), with the object's box drawn in the
// source's pixel grid, written in the sink's format; one launch for all sinks.  The arithmetic is exact integer (include/gen6d_hip.h,
// DESIGN.md §4.20) and is restated in numpy by tests/test_emit_source_cpu.py.  NV12 -> NV12 with one matrix is a pass-through: bytes no
// primitive covers are the source's bytes.
//
// Launch shape: that of frame_emit_kernel (emit.hip), whose drawing rules, cull and stores it shares through emit_common.h.  A sink is
// cut into 128 x 16 pixel tiles; blockIdx.x = sink * tiles + tile with `tiles` the tile count of the max_w x max_h the caller bounds the
// sinks by (a larger sink is walked with that stride); 256 threads, thread = 4 consecutive pixels of 2 consecutive rows = two whole
// chroma blocks.  Wave 0 culls the 12 edges and 8 discs against the tile into an LDS list.  A tile with an empty list (almost every
// tile) copies: the pass-through moves one Y dword per row and one UV dword per thread, every other pair converts and stores.  Source
// planes are arbitrarily aligned (a pitch can be odd, a device frame can start anywhere): the dword path is taken per thread and row
// only where the address is dword-aligned, bytes otherwise.  A thread's pixels are scalar words; no scratch (tests/test_emit_source_cpu.py).
// A block whose frame or sink has a format after NV12 or a full-range matrix runs ext_pixels (second half of the namespace, DESIGN.md
// §4.25): the same steps over the wider format set, with the pass-through for every same-format, same-matrix 8-bit YUV pair.
#include "emit_common.h"

namespace {

// 4 bytes at p, the first `cnt` of them inside the picture (the others come from `fill`): one dword where the address allows
__device__ __forceinline__ unsigned get4(const unsigned char* p, int cnt, unsigned fill) {
  if (cnt <= 0) return fill;
  if (cnt >= 4 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const unsigned*>(p);
  unsigned w = (fill & ~0xffu) | p[0];
  if (cnt > 1) w = (w & ~0xff00u) | ((unsigned)p[1] << 8);
  if (cnt > 2) w = (w & ~0xff0000u) | ((unsigned)p[2] << 16);
  if (cnt > 3) w = (w & ~0xff000000u) | ((unsigned)p[3] << 24);
  return w;
}
// 4 packed 3-byte pixels at s, the first `cnt` inside the picture (black outside), in memory order; three dword loads where the address allows
__device__ __forceinline__ Row load12(const unsigned char* s, int cnt) {
  Row r{0u, 0u, 0u, 0u};
  if (cnt <= 0) return r;
  if (cnt >= 4 && (reinterpret_cast<uintptr_t>(s) & 3u) == 0) {
    const unsigned* s32 = reinterpret_cast<const unsigned*>(s);
    const unsigned w0 = s32[0], w1 = s32[1], w2 = s32[2];
    r.a = w0 & 0xffffffu; r.b = (w0 >> 24) | ((w1 & 0xffffu) << 8); r.c = (w1 >> 16) | ((w2 & 0xffu) << 16); r.d = w2 >> 8;
  } else {
    r.a = pixel(s, true); r.b = pixel(s + 3, cnt > 1); r.c = pixel(s + 6, cnt > 2); r.d = pixel(s + 9, cnt > 3);
  }
  return r;
}
// 4 packed 4-byte pixels (the alpha is dropped); one dwordx4 or four dword loads where the address allows
__device__ __forceinline__ Row load16(const unsigned char* s, int cnt) {
  Row r{0u, 0u, 0u, 0u};
  if (cnt <= 0) return r;
  const uintptr_t al = reinterpret_cast<uintptr_t>(s);
  if (cnt >= 4 && (al & 15u) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(s);
    r.a = v.x & 0xffffffu; r.b = v.y & 0xffffffu; r.c = v.z & 0xffffffu; r.d = v.w & 0xffffffu;
  } else if ((al & 3u) == 0) {
    const unsigned* s32 = reinterpret_cast<const unsigned*>(s);
    r.a = s32[0] & 0xffffffu;
    if (cnt > 1) r.b = s32[1] & 0xffffffu;
    if (cnt > 2) r.c = s32[2] & 0xffffffu;
    if (cnt > 3) r.d = s32[3] & 0xffffffu;
  } else {
    r.a = pixel(s, true); r.b = pixel(s + 4, cnt > 1); r.c = pixel(s + 8, cnt > 2); r.d = pixel(s + 12, cnt > 3);
  }
  return r;
}

// round(k * 2^20) of a limited-range inverse matrix (the ingest's tap rule, header)
struct Inv { int cvr, cug, cvg, cub; };
// sat8(v >> 20), clamped BEFORE the shift.  Written as shift-then-clamp, the hipcc of ROCm 7.2 fuses two of them into v_ashr_pk_u8_i32 and ORs the B
// byte into its result as if the instruction cleared bits 16..31, which gfx950 does not do: B came out as garbage on the device
// (tests/test_emit_source_cpu.py pins that the instruction is absent from this kernel).
__device__ __forceinline__ unsigned sat8s20(int v) { return (unsigned)(min(max(v, 0), (256 << 20) - 1) >> 20); }
// one UV pair (low 16 bits of uv) and the two Y bytes above it (low 16 bits of y) -> two RGB pixels
// (TWIN: yuv8_pair below, the same formula for either range; a change of the rule goes into both)
__device__ __forceinline__ void nv12_pair(unsigned y, unsigned uv, const Inv& m, unsigned& p, unsigned& q) {
  const int d = (int)(uv & 255u) - 128, e = (int)((uv >> 8) & 255u) - 128;
  const int kr = m.cvr * e + (1 << 19), kg = -m.cug * d - m.cvg * e + (1 << 19), kb = m.cub * d + (1 << 19);
  const int c0 = max((int)(y & 255u) - 16, 0) * 1220542, c1 = max((int)((y >> 8) & 255u) - 16, 0) * 1220542;
  p = sat8s20(c0 + kr) | (sat8s20(c0 + kg) << 8) | (sat8s20(c0 + kb) << 16);
  q = sat8s20(c1 + kr) | (sat8s20(c1 + kg) << 8) | (sat8s20(c1 + kb) << 16);
}
__device__ __forceinline__ Row nv12_row(unsigned y, unsigned uv, const Inv& m) {
  Row r;
  nv12_pair(y, uv, m, r.a, r.b);
  nv12_pair(y >> 16, uv >> 16, m, r.c, r.d);
  return r;
}
// bit i of c set -> byte i of the result 0xff
__device__ __forceinline__ unsigned byte_mask(unsigned c) {
  return ((c & 1u) ? 0xffu : 0u) | ((c & 2u) ? 0xff00u : 0u) | ((c & 4u) ? 0xff0000u : 0u) | ((c & 8u) ? 0xff000000u : 0u);
}

// ---- frames and sinks of the formats after NV12 and of the full-range matrices (header) ----
// A block whose frame or sink is one of them takes ext_pixels (block-uniform); every other block runs the kernel's body as it was measured.
__device__ __forceinline__ bool extended_frame(const G6dFrame& f) { return f.format > G6D_FMT_NV12 || (f.format == G6D_FMT_NV12 && f.matrix > 1); }
__device__ __forceinline__ bool yuv8(int fmt) { return fmt >= G6D_FMT_NV12 && fmt <= G6D_FMT_YV12; }
__device__ __forceinline__ bool is422(int fmt) { return fmt == G6D_FMT_YUYV422 || fmt == G6D_FMT_UYVY422; }

// an inverse matrix of either range: c = max(Y - yoff, 0) * cy (yoff in 8-bit units; P010 subtracts 4 yoff)
struct InvX { int cy, yoff, cvr, cug, cvg, cub; };
__device__ __forceinline__ InvX inverse_matrix_x(int m) {
  const bool m709 = (m & 1) != 0;
  if (m >= 2) return InvX{1 << 20, 0, m709 ? 1651297 : 1470104, m709 ? 196424 : 360853, m709 ? 490864 : 748826, m709 ? 1945738 : 1858077};
  return InvX{1220542, 16, m709 ? 1880097 : 1673527, m709 ? 223347 : 409993, m709 ? 558891 : 852492, m709 ? 2214593 : 2116026};
}
// nv12_row for either range: 4 Y bytes and their chroma U0 V0 U1 V1 -> four RGB pixels (TWIN of nv12_pair / nv12_row above)
__device__ __forceinline__ void yuv8_pair(unsigned y, unsigned uv, const InvX& m, unsigned& p, unsigned& q) {
  const int d = (int)(uv & 255u) - 128, e = (int)((uv >> 8) & 255u) - 128;
  const int kr = m.cvr * e + (1 << 19), kg = -m.cug * d - m.cvg * e + (1 << 19), kb = m.cub * d + (1 << 19);
  const int c0 = max((int)(y & 255u) - m.yoff, 0) * m.cy, c1 = max((int)((y >> 8) & 255u) - m.yoff, 0) * m.cy;
  p = sat8s20(c0 + kr) | (sat8s20(c0 + kg) << 8) | (sat8s20(c0 + kb) << 16);
  q = sat8s20(c1 + kr) | (sat8s20(c1 + kg) << 8) | (sat8s20(c1 + kb) << 16);
}
__device__ __forceinline__ Row yuv8_row(unsigned y, unsigned uv, const InvX& m) {
  Row r;
  yuv8_pair(y, uv, m, r.a, r.b);
  yuv8_pair(y >> 16, uv >> 16, m, r.c, r.d);
  return r;
}
// 2 bytes at p, the first `cnt` of them inside the picture
__device__ __forceinline__ unsigned get2(const unsigned char* p, int cnt, unsigned fill) {
  if (cnt <= 0) return fill;
  unsigned w = (fill & ~0xffu) | p[0];
  if (cnt > 1) w = (w & 0xffu) | ((unsigned)p[1] << 8);
  return w;
}
// The raw samples of a thread's pixels (X .. X+3 of rows Y, Y+1) of an 8-bit YUV frame: y0 / y1 the Y bytes, c0 / c1 the chroma
// U0 V0 U1 V1 of the two rows (4:2:0: the same block row twice).  cnt0 / cnt1: source pixels of the row from X on (<= 0: the row lies
// outside the picture).  Outside the picture: yb (what black converts to: 16 limited, 0 full range) and 128.
struct Raw { unsigned y0, y1, c0, c1; };
__device__ __forceinline__ Raw load_yuv8(const G6dFrame& f, int X, int Y, int cnt0, int cnt1, unsigned yb) {
  const unsigned char* const s0 = static_cast<const unsigned char*>(f.plane0);
  const unsigned char* const s1 = static_cast<const unsigned char*>(f.plane1);
  const int fmt = f.format;
  const unsigned yfill = yb * 0x01010101u;
  Raw w;
  if (is422(fmt)) {                            // (block-uniform, as every format test here)
    const bool uyvy = fmt == G6D_FMT_UYVY422;
    const unsigned fy = yb | 0x8000u | (yb << 16) | 0x80000000u, fill = uyvy ? swap_bytes(fy) : fy;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cnt = j ? cnt1 : cnt0;
      const unsigned char* p = s0 + (size_t)(Y + j) * f.pitch0 + (size_t)X * 2;
      unsigned a = get4(p, 2 * cnt, fill), b = get4(p + 4, 2 * cnt - 4, fill);
      if (uyvy) { a = swap_bytes(a); b = swap_bytes(b); }
      const unsigned y = (a & 255u) | (((a >> 16) & 255u) << 8) | ((b & 255u) << 16) | (((b >> 16) & 255u) << 24);
      const unsigned c = ((a >> 8) & 255u) | ((a >> 24) << 8) | (((b >> 8) & 255u) << 16) | ((b >> 24) << 24);
      if (j) { w.y1 = y; w.c1 = c; } else { w.y0 = y; w.c0 = c; }
    }
    return w;
  }
  w.y0 = get4(s0 + (size_t)Y * f.pitch0 + X, cnt0, yfill);
  w.y1 = get4(s0 + (size_t)(Y + 1) * f.pitch0 + X, cnt1, yfill);
  if (fmt == G6D_FMT_NV12) {
    w.c0 = get4(s1 + (size_t)(Y >> 1) * f.pitch1 + X, cnt0, 0x80808080u);     // (even sizes: a chroma block is inside whole or not at all)
  } else {                                     // I420 / YV12: two bytes of each chroma plane
    const unsigned char* const second = s1 + (size_t)f.pitch1 * (f.height >> 1);
    const size_t o = (size_t)(Y >> 1) * f.pitch1 + (X >> 1);
    const int pairs = cnt0 >> 1;
    const unsigned u = get2((fmt == G6D_FMT_I420 ? s1 : second) + o, pairs, 0x8080u);
    const unsigned v = get2((fmt == G6D_FMT_I420 ? second : s1) + o, pairs, 0x8080u);
    w.c0 = (u & 255u) | ((v & 255u) << 8) | ((u >> 8) << 16) | ((v >> 8) << 24);
  }
  w.c1 = w.c0;
  return w;
}
// P010: pixels (X .. X+3, y), the first `cnt` inside the picture (black outside); the header's 64-bit sums, clamped before the shift
__device__ __forceinline__ unsigned ld10(const unsigned char* p) { return ((unsigned)p[0] | ((unsigned)p[1] << 8)) >> 6; }
__device__ __forceinline__ unsigned sat8s22(long long v) { return (unsigned)(min(max(v, 0LL), (256LL << 22) - 1) >> 22); }
// one chroma pair (4 bytes at pc) and the two luma samples under it (4 bytes at py) -> two RGB pixels
__device__ __forceinline__ void p010_pair(const unsigned char* py, const unsigned char* pc, const InvX& m, unsigned& p, unsigned& q) {
  const long long d = (long long)ld10(pc) - 512, e = (long long)ld10(pc + 2) - 512;
  const long long kr = m.cvr * e + (1 << 21), kg = -m.cug * d - m.cvg * e + (1 << 21), kb = m.cub * d + (1 << 21);
  const long long c0 = (long long)max((int)ld10(py) - 4 * m.yoff, 0) * m.cy, c1 = (long long)max((int)ld10(py + 2) - 4 * m.yoff, 0) * m.cy;
  p = sat8s22(c0 + kr) | (sat8s22(c0 + kg) << 8) | (sat8s22(c0 + kb) << 16);
  q = sat8s22(c1 + kr) | (sat8s22(c1 + kg) << 8) | (sat8s22(c1 + kb) << 16);
}
__device__ __forceinline__ Row p010_row(const G6dFrame& f, int X, int y, int cnt, const InvX& m) {
  Row r{0u, 0u, 0u, 0u};
  const unsigned char* const py = static_cast<const unsigned char*>(f.plane0) + (size_t)y * f.pitch0 + (size_t)X * 2;
  const unsigned char* const pc = static_cast<const unsigned char*>(f.plane1) + (size_t)(y >> 1) * f.pitch1 + (size_t)X * 2;
  if (cnt > 0) p010_pair(py, pc, m, r.a, r.b);             // (even widths: a pair is inside whole or not at all)
  if (cnt > 2) p010_pair(py + 4, pc + 4, m, r.c, r.d);
  return r;
}
__device__ __forceinline__ Row gray_row(const G6dFrame& f, int X, int y, int cnt) {
  const unsigned w = get4(static_cast<const unsigned char*>(f.plane0) + (size_t)y * f.pitch0 + X, cnt, 0u);
  return Row{(w & 255u) * 0x010101u, ((w >> 8) & 255u) * 0x010101u, ((w >> 16) & 255u) * 0x010101u, (w >> 24) * 0x010101u};
}

// A thread's pixels (X .. X+3 of rows Y, Y+1) of a block whose frame or sink is extended: the kernel's body with the wider format set.
// (TWIN of the body of frame_emit_source_kernel's second loop: the RGB loads, the cover / paint step and the pass-through merge are the
// same steps and must stay in step; tests/test_pixel_formats_gpu.py compares both against one restatement.)
// The pass-through holds for a frame and a sink of the same 8-bit YUV format and the same matrix value; its chroma block is 2 x 2
// for 4:2:0 and 2 x 1 for 4:2:2.
__device__ __forceinline__ void ext_pixels(const G6dSink& k, const G6dFrame& f, const int (*sp)[4], int ne, int n, int X, int Y, int pw, int ph,
                                           long long th2, int rad2, unsigned line, unsigned dot) {
  const int sfmt = f.format, kfmt = k.format;
  const int c0 = Y < ph ? pw - X : 0, c1 = Y + 1 < ph ? pw - X : 0;          // source pixels of the two rows from X on
  const bool pass = yuv8(sfmt) && sfmt == kfmt && f.matrix == k.matrix;
  const InvX inv = inverse_matrix_x(f.matrix);
  const FwdX fwd = forward_matrix_x(k.matrix);
  Raw raw{0u, 0u, 0u, 0u};
  Row r0{0u, 0u, 0u, 0u}, r1{0u, 0u, 0u, 0u};
  if (yuv8(sfmt)) {
    raw = load_yuv8(f, X, Y, c0, c1, (unsigned)inv.yoff);
    if (pass && n == 0) { store_yuv8(k, X, Y, raw.y0, raw.y1, raw.c0, raw.c1); return; }   // the copy: nothing is converted
    r0 = yuv8_row(raw.y0, raw.c0, inv); r1 = yuv8_row(raw.y1, raw.c1, inv);
  } else if (sfmt == G6D_FMT_P010) {
    r0 = p010_row(f, X, Y, c0, inv); r1 = p010_row(f, X, Y + 1, c1, inv);
  } else if (sfmt == G6D_FMT_GRAY8) {
    r0 = gray_row(f, X, Y, c0); r1 = gray_row(f, X, Y + 1, c1);
  } else {
    const unsigned char* const s0 = static_cast<const unsigned char*>(f.plane0);
    if (sfmt == G6D_FMT_RGB24 || sfmt == G6D_FMT_BGR24) {
      r0 = load12(s0 + (size_t)Y * f.pitch0 + (size_t)X * 3, c0); r1 = load12(s0 + (size_t)(Y + 1) * f.pitch0 + (size_t)X * 3, c1);
    } else {
      r0 = load16(s0 + (size_t)Y * f.pitch0 + (size_t)X * 4, c0); r1 = load16(s0 + (size_t)(Y + 1) * f.pitch0 + (size_t)X * 4, c1);
    }
    if (sfmt == G6D_FMT_BGR24 || sfmt == G6D_FMT_BGRA32) { swap_rb(r0); swap_rb(r1); }
  }
  unsigned m0 = 0, m1 = 0;                     // covered pixels of the two rows
  if (n > 0) {                                 // (block-uniform) listed primitives only
    unsigned e0 = 0, e1 = 0, d0 = 0, d1 = 0;
    cover(sp, ne, n, X, Y, th2, rad2, e0, e1, d0, d1);
    const unsigned in = c0 >= 4 ? 15u : (c0 > 0 ? (1u << c0) - 1u : 0u);     // pixels inside the picture
    const unsigned in0 = in, in1 = c1 > 0 ? in : 0u;
    paint(r0, e0 & in0, d0 & in0, line, dot);
    paint(r1, e1 & in1, d1 & in1, line, dot);
    m0 = (e0 | d0) & in0; m1 = (e1 | d1) & in1;
  }
  if (pass) {                                  // covered Y bytes and touched chroma blocks from the forward formulas, the rest raw
    const unsigned b0 = byte_mask(m0), b1 = byte_mask(m1);
    const unsigned y0 = (luma4_x(r0, fwd) & b0) | (raw.y0 & ~b0), y1 = (luma4_x(r1, fwd) & b1) | (raw.y1 & ~b1);
    if (is422(kfmt)) {
      const unsigned u0 = ((m0 & 3u) ? 0xffffu : 0u) | ((m0 & 12u) ? 0xffff0000u : 0u), u1 = ((m1 & 3u) ? 0xffffu : 0u) | ((m1 & 12u) ? 0xffff0000u : 0u);
      store_yuv8(k, X, Y, y0, y1, (chroma422_x(r0, fwd.m) & u0) | (raw.c0 & ~u0), (chroma422_x(r1, fwd.m) & u1) | (raw.c1 & ~u1));
    } else {
      const unsigned mb = m0 | m1, bu = ((mb & 3u) ? 0xffffu : 0u) | ((mb & 12u) ? 0xffff0000u : 0u);
      const unsigned c = (chroma420_x(r0, r1, fwd.m) & bu) | (raw.c0 & ~bu);
      store_yuv8(k, X, Y, y0, y1, c, c);
    }
  } else if (extended_sink(k)) {
    store_rows_x(k, r0, r1, X, Y, fwd);
  } else {
    store_rows(k, r0, r1, X, Y, fwd.m);
  }
}

__global__ void __launch_bounds__(256) frame_emit_source_kernel(const G6dSink* __restrict__ sinks, const G6dFrame* __restrict__ frames, int nf,
                                                                const int* __restrict__ pts, const int* __restrict__ valid, int sets, int B,
                                                                int tiles) {
  __shared__ int sp[20][4];                    // listed primitives: edges (ax, ay, bx, by) first, then discs (qx, qy, -, -)
  __shared__ int sn[2];                        // listed edges, listed primitives
  const int si = blockIdx.x / tiles, tile0 = blockIdx.x - si * tiles;
  const G6dSink& k = sinks[si];
  const int fi = k.slot, sw = k.width, sh = k.height;
  if (fi < 0 || fi >= nf || sw < 1 || sh < 1) return;     // (block-uniform)
  const G6dFrame& f = frames[fi];
  const int t = threadIdx.x;
  const int tiles_x = (sw + TW - 1) / TW, ntiles = tiles_x * ((sh + TH - 1) / TH);
  const int pw = max(f.width, 0), ph = max(f.height, 0);  // the picture is the whole source
  const int slot = f.slot, th = k.thickness, rad = k.dot_radius;
  const bool draw = (k.box == 0 || k.box == 1) && k.box < sets && slot >= 0 && slot < B && valid[(size_t)k.box * B + slot] != 0;
  const int* q = pts + (draw ? ((size_t)k.box * B + slot) * 16 : 0);
  const long long th2 = (long long)th * th;
  const int rad2 = rad * rad;
  const unsigned line = swap1((unsigned)k.line_rgb & 0xffffffu), dot = swap1((unsigned)k.dot_rgb & 0xffffffu);   // 0xRRGGBB -> Row order
  if (extended_frame(f) || extended_sink(k)) {             // (block-uniform) a tile walk of its own: neither loop carries the other's constants
    for (int tile = tile0; tile < ntiles; tile += tiles) {
      const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
      if (t < 64) cull_tile(sp, sn, t, draw, q, th, th2, rad, X0, Y0, pw, ph);
      __syncthreads();
      const int X = X0 + ((t & 31) << 2), Y = Y0 + ((t >> 5) << 1);
      if (X < sw && Y < sh) ext_pixels(k, f, sp, sn[0], sn[1], X, Y, pw, ph, th2, rad2, line, dot);
      __syncthreads();
    }
    return;
  }
  const unsigned char* const s0 = static_cast<const unsigned char*>(f.plane0);
  const unsigned char* const s1 = static_cast<const unsigned char*>(f.plane1);
  const int sfmt = f.format;
  const bool snv12 = sfmt == G6D_FMT_NV12, sswap = sfmt == G6D_FMT_BGR24 || sfmt == G6D_FMT_BGRA32;
  const bool pass = snv12 && k.format == G6D_FMT_NV12 && (f.matrix == 1) == (k.matrix == 1);
  const bool s709 = f.matrix == 1;
  const Inv inv{s709 ? 1880097 : 1673527, s709 ? 223347 : 409993, s709 ? 558891 : 852492, s709 ? 2214593 : 2116026};
  const Fwd fwd = forward_matrix(k.matrix == 1);

  for (int tile = tile0; tile < ntiles; tile += tiles) {   // (block-uniform trip count)
    const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
    if (t < 64) cull_tile(sp, sn, t, draw, q, th, th2, rad, X0, Y0, pw, ph);   // wave 0: the tile's primitive list
    __syncthreads();
    const int X = X0 + ((t & 31) << 2), Y = Y0 + ((t >> 5) << 1);
    if (X < sw && Y < sh) {
      const int ne = sn[0], n = sn[1];
      const int c0 = Y < ph ? pw - X : 0, c1 = Y + 1 < ph ? pw - X : 0;        // source pixels of the two rows from X on
      unsigned yw0 = 0, yw1 = 0, uvw = 0;      // NV12 source: the raw bytes; outside the picture what black converts to
      Row r0{0u, 0u, 0u, 0u}, r1{0u, 0u, 0u, 0u};
      if (snv12) {                             // (block-uniform)
        yw0 = get4(s0 + (size_t)Y * f.pitch0 + X, c0, 0x10101010u);
        yw1 = get4(s0 + (size_t)(Y + 1) * f.pitch0 + X, c1, 0x10101010u);
        uvw = get4(s1 + (size_t)(Y >> 1) * f.pitch1 + X, c0, 0x80808080u);     // (even sizes: a chroma block is inside whole or not at all)
      } else if (sfmt == G6D_FMT_RGB24 || sfmt == G6D_FMT_BGR24) {
        r0 = load12(s0 + (size_t)Y * f.pitch0 + (size_t)X * 3, c0);
        r1 = load12(s0 + (size_t)(Y + 1) * f.pitch0 + (size_t)X * 3, c1);
      } else {
        r0 = load16(s0 + (size_t)Y * f.pitch0 + (size_t)X * 4, c0);
        r1 = load16(s0 + (size_t)(Y + 1) * f.pitch0 + (size_t)X * 4, c1);
      }
      if (pass && n == 0) {                    // (block-uniform) the copy: nothing is converted
        const bool full = X + 4 <= sw;
        put4(static_cast<unsigned char*>(k.plane0) + (size_t)Y * k.pitch0 + X, yw0, full, sw - X);
        if (Y + 1 < sh) {
          put4(static_cast<unsigned char*>(k.plane0) + (size_t)(Y + 1) * k.pitch0 + X, yw1, full, sw - X);
          put4(static_cast<unsigned char*>(k.plane1) + (size_t)(Y >> 1) * k.pitch1 + X, uvw, full, sw - X);
        }
      } else {
        if (snv12) { r0 = nv12_row(yw0, uvw, inv); r1 = nv12_row(yw1, uvw, inv); }
        else if (sswap) { swap_rb(r0); swap_rb(r1); }
        unsigned m0 = 0, m1 = 0;               // covered pixels of the two rows
        if (n > 0) {                           // (block-uniform) listed primitives only
          unsigned e0 = 0, e1 = 0, d0 = 0, d1 = 0;
          cover(sp, ne, n, X, Y, th2, rad2, e0, e1, d0, d1);
          const unsigned in = c0 >= 4 ? 15u : (c0 > 0 ? (1u << c0) - 1u : 0u);           // pixels inside the picture
          const unsigned in0 = in, in1 = c1 > 0 ? in : 0u;
          paint(r0, e0 & in0, d0 & in0, line, dot);
          paint(r1, e1 & in1, d1 & in1, line, dot);
          m0 = (e0 | d0) & in0; m1 = (e1 | d1) & in1;
        }
        if (pass) {                            // (block-uniform) covered Y bytes and touched UV pairs from the forward formulas, the rest raw
          const bool full = X + 4 <= sw;
          const unsigned b0 = byte_mask(m0), b1 = byte_mask(m1), mb = m0 | m1;
          const unsigned bu = ((mb & 3u) ? 0xffffu : 0u) | ((mb & 12u) ? 0xffff0000u : 0u);
          put4(static_cast<unsigned char*>(k.plane0) + (size_t)Y * k.pitch0 + X, (luma4(r0, fwd) & b0) | (yw0 & ~b0), full, sw - X);
          if (Y + 1 < sh) {
            put4(static_cast<unsigned char*>(k.plane0) + (size_t)(Y + 1) * k.pitch0 + X, (luma4(r1, fwd) & b1) | (yw1 & ~b1), full, sw - X);
            put4(static_cast<unsigned char*>(k.plane1) + (size_t)(Y >> 1) * k.pitch1 + X, (chroma4(r0, r1, fwd) & bu) | (uvw & ~bu), full,
                 sw - X);
          }
        } else {
          store_rows(k, r0, r1, X, Y, fwd);
        }
      }
    }
    __syncthreads();                                       // the list is rebuilt for the next tile of a sink larger than max_w x max_h
  }
}

}  // namespace

extern "C" int g6d_frame_emit_source(const G6dSink* sinks, int n, const G6dFrame* frames, int nf, const int32_t* pts, const int32_t* valid,
                                     int sets, int B, int max_w, int max_h, g6d_stream_t stream) {
  if (!sinks || n < 0 || !frames || nf < 1 || !pts || !valid || sets < 1 || sets > 2 || B < 1 || max_w < 1 || max_h < 1 || max_w > 8192 ||
      max_h > 8192) {
    g6d_set_error("frame_emit_source: bad args (null table / frames / pts / valid, n < 0, nf < 1, sets not 1 or 2, B < 1 or max_w, max_h "
                  "outside 1..8192)");
    return G6D_EINVAL;
  }
  if (n == 0) return G6D_OK;
  const int tiles = ((max_w + TW - 1) / TW) * ((max_h + TH - 1) / TH);
  if ((long long)tiles * n > 0x7fffffffLL) { g6d_set_error("frame_emit_source: too many tiles for one launch"); return G6D_EINVAL; }
  hipLaunchKernelGGL(frame_emit_source_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), sinks, frames,
                     nf, pts, valid, sets, B, tiles);
  return g6d_check_launch("frame_emit_source");
}
