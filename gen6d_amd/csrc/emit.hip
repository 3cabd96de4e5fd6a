// Annotated frame output (gen6d_amd/emit.py; reference predict.py:60-72 + utils/draw_utils.py draw_bbox_3d): the working-resolution RGB
// images of a batch, with the object's projected box drawn on them, written in an encoder's or a display's format (packed RGB / BGR(A),
// NV12) into buffers the caller names; one launch for all sinks.  The arithmetic is exact integer (include/gen6d_hip.h)
// and is restated in numpy by tests/test_emit_cpu.py.
//
// Launch shape: a sink is cut into 128 x 16 pixel tiles; block = tiles of one sink (flat list: blockIdx.x = sink * tiles + tile, where
// `tiles` is the tile count of the H x W canvas; a sink with more tiles than the canvas is walked with that stride), 256 threads,
// thread = 4 consecutive pixels of 2 consecutive rows, i.e. two whole NV12 chroma blocks: no chroma block straddles threads.  A wave
// covers 4 rows x 128 pixels.  Per tile, wave 0 culls the 12 edges and 8 discs against the tile's pixel rectangle (bounding boxes grown by
// the half thickness / radius, and the edge's supporting line against the rectangle's corners) into an LDS list; the cull is
// block-uniform.  A tile with an empty list (almost every tile) is a convert-and-copy: three dword loads per thread and row where the
// canvas rows are dword-aligned, dword / dwordx4 stores where the sink's are.  Only listed primitives are tested per pixel.  A thread's
// 8 pixels live in 8 scalar words (a byte array here was moved to LDS by the compiler); no scratch (tests/test_emit_cpu.py).
#include "g6d_common.h"
#include "pose_algebra.h"

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
// picture pixels (X .. X+3, y) of image `slot`, black outside the pw x ph picture; three dword loads where the address allows
__device__ __forceinline__ Row fill_row(const unsigned char* __restrict__ imgs, int slot, int H, int W, int X, int y, int pw, int ph) {
  Row r{0u, 0u, 0u, 0u};
  if (y >= ph || X >= pw) return r;
  const unsigned char* src = imgs + (((size_t)slot * H + y) * W + X) * 3;
  if (X + 4 <= pw && (reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
    const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
    const unsigned w0 = s32[0], w1 = s32[1], w2 = s32[2];
    r.a = w0 & 0xffffffu; r.b = (w0 >> 24) | ((w1 & 0xffffu) << 8); r.c = (w1 >> 16) | ((w2 & 0xffu) << 16); r.d = w2 >> 8;
  } else {
    r.a = pixel(src, true); r.b = pixel(src + 3, X + 1 < pw); r.c = pixel(src + 6, X + 2 < pw); r.d = pixel(src + 9, X + 3 < pw);
  }
  return r;
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

__global__ void __launch_bounds__(256) frame_emit_kernel(const G6dSink* __restrict__ sinks, const unsigned char* __restrict__ imgs, int B,
                                                         int H, int W, const int* __restrict__ pts, const int* __restrict__ valid,
                                                         int tiles) {
  __shared__ int sp[20][4];                    // listed primitives: edges (ax, ay, bx, by) first, then discs (qx, qy, -, -)
  __shared__ int sn[2];                        // listed edges, listed primitives
  const int si = blockIdx.x / tiles, tile0 = blockIdx.x - si * tiles;
  const G6dSink& k = sinks[si];
  const int slot = k.slot, sw = k.width, sh = k.height;
  if (slot < 0 || slot >= B || sw < 1 || sh < 1) return;  // (block-uniform)
  const int t = threadIdx.x;
  const int tiles_x = (sw + TW - 1) / TW, ntiles = tiles_x * ((sh + TH - 1) / TH);
  const int pw = max(min(k.pic_w, W), 0), ph = max(min(k.pic_h, H), 0);
  const int fmt = k.format, th = k.thickness, rad = k.dot_radius;
  const bool draw = (k.box == 0 || k.box == 1) && valid[(size_t)k.box * B + slot] != 0;
  const int* q = pts + (draw ? ((size_t)k.box * B + slot) * 16 : 0);
  const long long th2 = (long long)th * th;
  const int rad2 = rad * rad;
  const unsigned line = swap1((unsigned)k.line_rgb & 0xffffffu), dot = swap1((unsigned)k.dot_rgb & 0xffffffu);   // 0xRRGGBB -> Row order
  unsigned char* const p0 = static_cast<unsigned char*>(k.plane0);
  unsigned char* const p1 = static_cast<unsigned char*>(k.plane1);
  const bool m709 = k.matrix == 1;
  const int cyr = m709 ? 191455 : 269262, cyg = m709 ? 644067 : 528618, cyb = m709 ? 65019 : 102662;
  const int cbr = m709 ? -105533 : -155423, cbg = m709 ? -355018 : -305128, cbb = 460551;
  const int crr = 460551, crg = m709 ? -418321 : -385654, crb = m709 ? -42230 : -74897;

  for (int tile = tile0; tile < ntiles; tile += tiles) {   // (block-uniform trip count)
    const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
    if (t < 64) {                                          // wave 0: the tile's primitive list
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
    __syncthreads();
    const int X = X0 + ((t & 31) << 2), Y = Y0 + ((t >> 5) << 1);
    if (X < sw && Y < sh) {
      const int ne = sn[0], n = sn[1];
      const bool full = X + 4 <= sw;
      Row r0 = fill_row(imgs, slot, H, W, X, Y, pw, ph), r1 = fill_row(imgs, slot, H, W, X, Y + 1, pw, ph);
      if (n > 0) {                                         // (block-uniform) listed primitives only; bit i of a mask = pixel X + i
        unsigned e0 = 0, e1 = 0, d0 = 0, d1 = 0;
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
        const unsigned in = X + 4 <= pw ? 15u : (X < pw ? (1u << (pw - X)) - 1u : 0u);      // pixels inside the picture
        const unsigned in0 = Y < ph ? in : 0u, in1 = Y + 1 < ph ? in : 0u;
        paint(r0, e0 & in0, d0 & in0, line, dot);
        paint(r1, e1 & in1, d1 & in1, line, dot);
      }
      if (fmt == G6D_FMT_NV12) {                           // (block-uniform)
        const unsigned y0 = luma(r0.a, cyr, cyg, cyb) | (luma(r0.b, cyr, cyg, cyb) << 8) | (luma(r0.c, cyr, cyg, cyb) << 16) |
                            (luma(r0.d, cyr, cyg, cyb) << 24);
        const unsigned y1 = luma(r1.a, cyr, cyg, cyb) | (luma(r1.b, cyr, cyg, cyb) << 8) | (luma(r1.c, cyr, cyg, cyb) << 16) |
                            (luma(r1.d, cyr, cyg, cyb) << 24);
        put4(p0 + (size_t)Y * k.pitch0 + X, y0, full, sw - X);
        if (Y + 1 < sh) {
          put4(p0 + (size_t)(Y + 1) * k.pitch0 + X, y1, full, sw - X);
          // channel sums of a 2 x 2 block: R | G << 8 | B << 16 of four pixels summed in 16-bit fields
          const unsigned lo0 = (r0.a & 0xff00ffu) + (r0.b & 0xff00ffu) + (r1.a & 0xff00ffu) + (r1.b & 0xff00ffu);
          const unsigned g0 = ((r0.a >> 8) & 255u) + ((r0.b >> 8) & 255u) + ((r1.a >> 8) & 255u) + ((r1.b >> 8) & 255u);
          const unsigned lo1 = (r0.c & 0xff00ffu) + (r0.d & 0xff00ffu) + (r1.c & 0xff00ffu) + (r1.d & 0xff00ffu);
          const unsigned g1 = ((r0.c >> 8) & 255u) + ((r0.d >> 8) & 255u) + ((r1.c >> 8) & 255u) + ((r1.d >> 8) & 255u);
          const int sr0 = lo0 & 0xffff, sb0 = lo0 >> 16, sr1 = lo1 & 0xffff, sb1 = lo1 >> 16;
          const unsigned uv = (unsigned)sat8((cbr * sr0 + cbg * (int)g0 + cbb * sb0 + (1 << 21) + (128 << 22)) >> 22) |
                              ((unsigned)sat8((crr * sr0 + crg * (int)g0 + crb * sb0 + (1 << 21) + (128 << 22)) >> 22) << 8) |
                              ((unsigned)sat8((cbr * sr1 + cbg * (int)g1 + cbb * sb1 + (1 << 21) + (128 << 22)) >> 22) << 16) |
                              ((unsigned)sat8((crr * sr1 + crg * (int)g1 + crb * sb1 + (1 << 21) + (128 << 22)) >> 22) << 24);
          put4(p1 + (size_t)(Y >> 1) * k.pitch1 + X, uv, full, sw - X);     // (an even width: a chroma pair is inside whole or not at all)
        }
      } else {
        if (fmt == G6D_FMT_BGR24 || fmt == G6D_FMT_BGRA32) { swap_rb(r0); swap_rb(r1); }
        if (fmt == G6D_FMT_RGB24 || fmt == G6D_FMT_BGR24) {
          put12(p0 + (size_t)Y * k.pitch0 + (size_t)X * 3, r0, full, 3 * (sw - X));
          if (Y + 1 < sh) put12(p0 + (size_t)(Y + 1) * k.pitch0 + (size_t)X * 3, r1, full, 3 * (sw - X));
        } else {                                           // RGBA32 / BGRA32, alpha 255
          put16(p0 + (size_t)Y * k.pitch0 + (size_t)X * 4, r0, full, sw - X);
          if (Y + 1 < sh) put16(p0 + (size_t)(Y + 1) * k.pitch0 + (size_t)X * 4, r1, full, sw - X);
        }
      }
    }
    __syncthreads();                                       // the list is rebuilt for the next tile of a sink larger than the canvas
  }
}

// One 64-thread block per slot; lane l projects corner l & 7 (as track_commit_kernel), lanes 0..7 store.
__global__ void __launch_bounds__(64) track_corners_kernel(const float* __restrict__ table, const float* __restrict__ Ks,
                                                           const int* __restrict__ slot_stream, const float* __restrict__ box,
                                                           int* __restrict__ pts, int* __restrict__ valid) {
  using namespace pa;
  const int b = blockIdx.x, lane = threadIdx.x, c = lane & 7;
  const int s = slot_stream[b];
  bool ok = s >= 0;
  int qx = 0, qy = 0;
  if (ok) {
    P34 p; M3 K;
    for (int i = 0; i < 12; ++i) p.m[i] = table[(size_t)12 * s + i];
    for (int i = 0; i < 9; ++i) K.m[i] = Ks[9 * b + i];
    double u, v, d;
    project_point(V3{box[3 * c], box[3 * c + 1], box[3 * c + 2]}, p, K, u, v, d);
    const double fu = floor(u + 0.5), fv = floor(v + 0.5);
    ok = d > 0 && fu >= (double)QMIN && fu <= (double)QMAX && fv >= (double)QMIN && fv <= (double)QMAX;     // (NaN: false)
    if (ok) { qx = (int)fu; qy = (int)fv; }
  }
  const bool all = __ballot(ok) == ~0ull;
  if (lane < 8) { pts[(b * 8 + c) * 2] = all ? qx : 0; pts[(b * 8 + c) * 2 + 1] = all ? qy : 0; }
  if (lane == 0) valid[b] = all ? 1 : 0;
}

}  // namespace

extern "C" int g6d_sizeof_sink_desc(void) { return (int)sizeof(G6dSink); }

extern "C" int g6d_track_corners(const float* table, const float* K, const int* slot_stream, const float* box, int32_t* pts, int32_t* valid,
                                 int batch, g6d_stream_t stream) {
  if (!table || !K || !slot_stream || !box || !pts || !valid || batch < 1) { g6d_set_error("track_corners: bad args"); return G6D_EINVAL; }
  hipLaunchKernelGGL(track_corners_kernel, dim3(batch), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), table, K, slot_stream, box, pts,
                     valid);
  return g6d_check_launch("track_corners");
}

extern "C" int g6d_frame_emit(const G6dSink* sinks, int n, const uint8_t* imgs, int B, int H, int W, const int32_t* pts,
                              const int32_t* valid, g6d_stream_t stream) {
  if (!sinks || n < 0 || !imgs || !pts || !valid || B < 1 || H < 1 || W < 1) {
    g6d_set_error("frame_emit: bad args (null table / imgs / pts / valid, n < 0 or a non-positive canvas)"); return G6D_EINVAL;
  }
  if (n == 0) return G6D_OK;
  const int tiles = ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  if ((long long)tiles * n > 0x7fffffffLL) { g6d_set_error("frame_emit: too many tiles for one launch"); return G6D_EINVAL; }
  hipLaunchKernelGGL(frame_emit_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), sinks, imgs, B, H, W,
                     pts, valid, tiles);
  return g6d_check_launch("frame_emit");
}
