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
// Sinks of the formats after NV12 (I420 / YV12, YUYV422 / UYVY422) and of the full-range matrices walk their tiles in a loop of their own
// (block-uniform, ahead of the loop every other sink runs) and store through emit_common.h's store_rows_x.
#include "emit_common.h"
#include "pose_algebra.h"

namespace {

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

// The tile walk of an extended sink (TWIN of frame_emit_kernel's prologue and loop: the same box, style, cull, fill and paint steps, with
// emit_common.h's store_rows_x at the end; they must stay in step)
__device__ __forceinline__ void ext_walk(const G6dSink& k, const unsigned char* __restrict__ imgs, int B, int H, int W, const int* __restrict__ pts,
                                         const int* __restrict__ valid, int tile0, int tiles, int (*sp)[4], int* sn) {
  const int t = threadIdx.x, slot = k.slot, sw = k.width, sh = k.height;
  const int tiles_x = (sw + TW - 1) / TW, ntiles = tiles_x * ((sh + TH - 1) / TH);
  const int pw = max(min(k.pic_w, W), 0), ph = max(min(k.pic_h, H), 0);
  const int th = k.thickness, rad = k.dot_radius;
  const bool draw = (k.box == 0 || k.box == 1) && valid[(size_t)k.box * B + slot] != 0;
  const int* q = pts + (draw ? ((size_t)k.box * B + slot) * 16 : 0);
  const long long th2 = (long long)th * th;
  const int rad2 = rad * rad;
  const unsigned line = swap1((unsigned)k.line_rgb & 0xffffffu), dot = swap1((unsigned)k.dot_rgb & 0xffffffu);
  const FwdX fx = forward_matrix_x(k.matrix);
  for (int tile = tile0; tile < ntiles; tile += tiles) {   // (block-uniform trip count)
    const int X0 = (tile % tiles_x) * TW, Y0 = (tile / tiles_x) * TH;
    if (t < 64) cull_tile(sp, sn, t, draw, q, th, th2, rad, X0, Y0, pw, ph);
    __syncthreads();
    const int X = X0 + ((t & 31) << 2), Y = Y0 + ((t >> 5) << 1);
    if (X < sw && Y < sh) {
      const int ne = sn[0], n = sn[1];
      Row r0 = fill_row(imgs, slot, H, W, X, Y, pw, ph), r1 = fill_row(imgs, slot, H, W, X, Y + 1, pw, ph);
      if (n > 0) {
        unsigned e0 = 0, e1 = 0, d0 = 0, d1 = 0;
        cover(sp, ne, n, X, Y, th2, rad2, e0, e1, d0, d1);
        const unsigned in = X + 4 <= pw ? 15u : (X < pw ? (1u << (pw - X)) - 1u : 0u);
        const unsigned in0 = Y < ph ? in : 0u, in1 = Y + 1 < ph ? in : 0u;
        paint(r0, e0 & in0, d0 & in0, line, dot);
        paint(r1, e1 & in1, d1 & in1, line, dot);
      }
      store_rows_x(k, r0, r1, X, Y, fx);
    }
    __syncthreads();
  }
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
  // (block-uniform) A sink of the formats after NV12 or of a full-range matrix: a tile walk of its own, entered before anything below is
  // computed, so that the rest of this kernel is compiled from the lines and the live values it had before that walk existed
  if (extended_sink(k)) { ext_walk(k, imgs, B, H, W, pts, valid, tile0, tiles, sp, sn); return; }
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
    if (t < 64) cull_tile(sp, sn, t, draw, q, th, th2, rad, X0, Y0, pw, ph);   // wave 0: the tile's primitive list
    __syncthreads();
    const int X = X0 + ((t & 31) << 2), Y = Y0 + ((t >> 5) << 1);
    if (X < sw && Y < sh) {
      const int ne = sn[0], n = sn[1];
      const bool full = X + 4 <= sw;
      Row r0 = fill_row(imgs, slot, H, W, X, Y, pw, ph), r1 = fill_row(imgs, slot, H, W, X, Y + 1, pw, ph);
      if (n > 0) {                                         // (block-uniform) listed primitives only; bit i of a mask = pixel X + i
        unsigned e0 = 0, e1 = 0, d0 = 0, d1 = 0;
        cover(sp, ne, n, X, Y, th2, rad2, e0, e1, d0, d1);
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
  const long long tiles_ll = (((long long)W + TW - 1) / TW) * (((long long)H + TH - 1) / TH);      // (in 64 bits: the product of two ints)
  if ((long long)W + TW - 1 > 0x7fffffffLL || (long long)H + TH - 1 > 0x7fffffffLL || tiles_ll * n > 0x7fffffffLL) { g6d_set_error("frame_emit: too many tiles for one launch"); return G6D_EINVAL; }
  const int tiles = (int)tiles_ll;
  hipLaunchKernelGGL(frame_emit_kernel, dim3((unsigned)(tiles * n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), sinks, imgs, B, H, W,
                     pts, valid, tiles);
  return g6d_check_launch("frame_emit");
}
