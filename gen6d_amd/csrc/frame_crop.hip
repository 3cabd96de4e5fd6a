// Query crops cut from the camera-native frames (gen6d_amd/chain.py `query_batch_source`): g6d_warp_batch's crop of
// the working-resolution canvas, sampled in the SOURCE picture instead, through the crop homography composed with the inverse of the
// ingest's scaling and quarter turn.  One launch for a batch; slot b samples frames[rec[b]], or its canvas when rec[b] < 0 (no source: a
// lens frame, an unused slot), by g6d_warp_batch's rule bit for bit.  The rule is in include/gen6d_hip.h and is restated in numpy by
// tests/test_frame_crop_cpu.py.  Everything is read from device memory when the kernel runs, so the launch sits inside the tick's graph.
//
// Launch shape: the crop is cut into 64 x 4 pixel tiles; block = one tile of one slot (blockIdx.y = slot), 256 threads, thread = one crop
// pixel, a wave = 64 consecutive pixels of one crop row: each of its three plane stores is one 256-byte stretch, and where the crop
// magnifies the source neighbouring lanes read neighbouring source bytes.  rec[b], the record and the homography sit at block-uniform
// addresses (scalar loads, once per block), so the has-source, format and rotation branches are block-uniform.  The canvas is sampled as
// what it is, a same-size rgb24 picture of pitch 3 W: both branches run `taps_of` and `blend`, so they cannot drift apart.
// A frame of the formats after NV12 or of a full-range matrix takes its taps from frame_src.h's `ext_taps` (block-uniform).
#include "frame_src.h"

namespace {

constexpr int CW = 64, CH = 4;

// canvas pixel -> source pixel: the quarter turn undone (wt1 = wt - 1, ht1 = ht - 1), then f = p * a + b per axis; sw x sh is the source
struct View { int rot, sw, sh; float wt1, ht1, ax, bx, ay, by; };

__device__ __forceinline__ View view_of(const G6dFrame& f) {
  const bool swap = f.rotate == 90 || f.rotate == 270;
  const int wt = swap ? f.out_h : f.out_w, ht = swap ? f.out_w : f.out_h;
  View v;
  v.rot = f.rotate; v.sw = f.width; v.sh = f.height;
  v.wt1 = (float)(wt - 1); v.ht1 = (float)(ht - 1);
  v.ax = (float)f.width / (float)wt; v.bx = 0.5f * v.ax - 0.5f;
  v.ay = (float)f.height / (float)ht; v.by = 0.5f * v.ay - 0.5f;
  return v;
}

struct Taps { int x0, x1, y0, y1; float w00, w01, w10, w11; };

// crop pixel (x, y) -> the four taps (clamped into the source) and their weights (0 for a tap outside it): warp_batch_kernel's
// arithmetic (pose_chain.hip), with the view's map between the homography and the clamp.
// DEPENDENCY: warp_batch_kernel is compiled with the compiler's default contraction, which leaves it the choice of what to fuse in the
// homography's sums and in the blend.  Here contraction is off and the operations are spelled out the way hipcc compiles that kernel
// today (ROCm 7.0): the homography's products and sums rounded one by one, the blend as w01 p01 rounded, then one fused multiply-add
// each for w00, w10, w11.  This side is therefore fixed, the other is not: a compiler that fuses warp_batch_kernel differently breaks the
// bit equality of the rec < 0 slots, and only the torch.equal cases of tests/test_frame_crop_gpu.py would show it.  The lasting form
// is one device function for both kernels (or the same pragma there); it changes warp_batch_kernel's build and is left to a change
// of its own.
// (x, y are real numbers: g6d_frame_crop passes a pixel's integer coordinates, g6d_frame_crop_area the sample positions inside it.
// `pos_of` is steps 1 - 3 of the rule, the source position before the clamp, which the area crop also takes its footprint from)
__device__ __forceinline__ float2 pos_of(const float* __restrict__ h, float x, float y, const View& v) {
#pragma clang fp contract(off)
  const float X = h[0] * x + h[1] * y + h[2], Y = h[3] * x + h[4] * y + h[5], Wd = h[6] * x + h[7] * y + h[8];
  const float iw = Wd != 0.f ? 1.f / Wd : 0.f;
  const float cx = X * iw, cy = Y * iw;
  float px = cx, py = cy;
  if (v.rot == 90) { px = cy; py = v.ht1 - cx; }                      // (block-uniform)
  else if (v.rot == 180) { px = v.wt1 - cx; py = v.ht1 - cy; }
  else if (v.rot == 270) { px = v.wt1 - cy; py = cx; }
  return make_float2(fmaf(px, v.ax, v.bx), fmaf(py, v.ay, v.by));
}
__device__ __forceinline__ Taps taps_of(const float* __restrict__ h, float x, float y, const View& v) {
#pragma clang fp contract(off)
  const float2 p = pos_of(h, x, y, v);
  const int sw = v.sw, sh = v.sh;
  float fx = fminf(fmaxf(p.x, -4.f), (float)sw + 4.f), fy = fminf(fmaxf(p.y, -4.f), (float)sh + 4.f);
  const float x0f = floorf(fx), y0f = floorf(fy);
  const int x0 = (int)x0f, y0 = (int)y0f;
  const float ax = fx - x0f, ay = fy - y0f;
  const bool vx0 = (unsigned)x0 < (unsigned)sw, vx1 = (unsigned)(x0 + 1) < (unsigned)sw;
  const bool vy0 = (unsigned)y0 < (unsigned)sh, vy1 = (unsigned)(y0 + 1) < (unsigned)sh;
  Taps t;
  t.x0 = min(max(x0, 0), sw - 1); t.x1 = min(max(x0 + 1, 0), sw - 1);
  t.y0 = min(max(y0, 0), sh - 1); t.y1 = min(max(y0 + 1, 0), sh - 1);
  t.w00 = (vx0 && vy0) ? (1.f - ax) * (1.f - ay) : 0.f; t.w01 = (vx1 && vy0) ? ax * (1.f - ay) : 0.f;
  t.w10 = (vx0 && vy1) ? (1.f - ax) * ay : 0.f; t.w11 = (vx1 && vy1) ? ax * ay : 0.f;
  return t;
}

// the weighted sum of a sample's taps, unrounded, and what a destination value is made of such a sum
__device__ __forceinline__ float weighted(const Taps& t, int p00, int p01, int p10, int p11) {
#pragma clang fp contract(off)
  return fmaf(t.w11, (float)p11, fmaf(t.w10, (float)p10, fmaf(t.w00, (float)p00, t.w01 * (float)p01)));
}
__device__ __forceinline__ float level(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f) * (1.f / 255.f); }
__device__ __forceinline__ float blend(const Taps& t, int p00, int p01, int p10, int p11) { return level(weighted(t, p00, p01, p10, p11)); }

__global__ void __launch_bounds__(256) frame_crop_kernel(const G6dFrame* __restrict__ frames, const int* __restrict__ rec,
                                                        const unsigned char* __restrict__ imgs, int H, int W,
                                                        const float* __restrict__ hinv, float* __restrict__ dst, int dh, int dw, int tiles_x) {
  const int b = blockIdx.y;
  const int x = (blockIdx.x % tiles_x) * CW + (threadIdx.x & (CW - 1)), y = (blockIdx.x / tiles_x) * CH + threadIdx.x / CW;
  const int r = rec[b];
  Src s;
  View v;
  const bool ext = r >= 0 && extended(frames[r]);                     // (block-uniform) a format after NV12 or a full-range matrix
  if (r >= 0) {                                                       // (block-uniform)
    const G6dFrame& f = frames[r];
    s = source_of(f);
    v = view_of(f);
  } else {                                                            // the slot's canvas: an unturned rgb24 picture of its own size
    s.p0 = imgs + (size_t)b * H * W * 3; s.p1 = nullptr;
    s.pitch0 = 3 * W; s.pitch1 = 0; s.nv12 = 0; s.bpp = 3; s.ro = 0;
    s.cvr = s.cug = s.cvg = s.cub = 0;
    v.rot = 0; v.sw = W; v.sh = H; v.wt1 = v.ht1 = 0.f;
    v.ax = v.ay = 1.f; v.bx = v.by = 0.f;                             // f = p * 1 + 0 = p exactly
  }
  if (x >= dw || y >= dh) return;
  const Taps t = taps_of(hinv + 9 * b, x, y, v);
  int r00, g00, b00, r01, g01, b01, r10, g10, b10, r11, g11, b11;
  if (ext) {                                                          // every tap is taken, as below: a weight-0 tap is clamped inside the source
    Tap t00, t01, t10, t11;
    ext_taps<false>(yuv_of(frames[r]), t.x0, t.x1, t.y0, t.y1, true, true, t00, t01, t10, t11);
    r00 = t00.r; g00 = t00.g; b00 = t00.b; r01 = t01.r; g01 = t01.g; b01 = t01.b;
    r10 = t10.r; g10 = t10.g; b10 = t10.b; r11 = t11.r; g11 = t11.g; b11 = t11.b;
  } else if (s.nv12) {                                                       // (block-uniform) a UV sample is loaded once for the taps that share it
    const bool sx = (t.x1 >> 1) == (t.x0 >> 1), sy = (t.y1 >> 1) == (t.y0 >> 1);
    const Chroma k00 = chroma(s, t.x0 >> 1, t.y0 >> 1);
    const Chroma k01 = sx ? k00 : chroma(s, t.x1 >> 1, t.y0 >> 1);
    const Chroma k10 = sy ? k00 : chroma(s, t.x0 >> 1, t.y1 >> 1);
    const Chroma k11 = sx ? k10 : (sy ? k01 : chroma(s, t.x1 >> 1, t.y1 >> 1));
    tap_nv12(s, k00, t.x0, t.y0, r00, g00, b00); tap_nv12(s, k01, t.x1, t.y0, r01, g01, b01);
    tap_nv12(s, k10, t.x0, t.y1, r10, g10, b10); tap_nv12(s, k11, t.x1, t.y1, r11, g11, b11);
  } else {
    tap_packed(s, t.x0, t.y0, r00, g00, b00); tap_packed(s, t.x1, t.y0, r01, g01, b01);
    tap_packed(s, t.x0, t.y1, r10, g10, b10); tap_packed(s, t.x1, t.y1, r11, g11, b11);
  }
  const size_t plane = (size_t)dh * dw;
  float* o = dst + (size_t)b * 3 * plane + (size_t)y * dw + x;
  o[0] = blend(t, r00, r01, r10, r11);
  o[plane] = blend(t, g00, g01, g10, g11);
  o[2 * plane] = blend(t, b00, b01, b10, b11);
}

// ---- g6d_frame_crop_area: the crop supersampled n x n per pixel, n from the slot's own footprint (include/gen6d_hip.h) ----
// The same launch shape.  n is block-uniform: every thread derives it from the slot's homography and view (three evaluations of
// `pos_of` at the crop's centre), then runs n^2 samples through the `taps_of` and `weighted` of the kernel above.  With n = 1
// the one sample sits at the pixel's own coordinates, the sum is its weighted sum and the mean divides by 1: g6d_frame_crop's bits.
// frame_crop_kernel above stays as it was measured (§4.24); its slot set-up and its tap loads are restated here as functions for the area
// kernel (pulling them out of frame_crop_kernel changes its scalar prologue, as ingest.hip found for its kernel).  TWINS: a change of
// either goes into both; the torch.equal cases of tests/test_frame_crop_area_gpu.py (n = 1 against g6d_frame_crop) hold them together.
// What slot b samples: frames[r], or with r < 0 its canvas as an unturned rgb24 picture of its own size (all block-uniform)
struct Slot { Src s; View v; bool ext; };
__device__ __forceinline__ Slot slot_of(const G6dFrame* __restrict__ frames, int r, const unsigned char* __restrict__ imgs, int b, int H, int W) {
  Slot q;
  q.ext = r >= 0 && extended(frames[r]);                              // a format after NV12 or a full-range matrix
  if (r >= 0) {
    const G6dFrame& f = frames[r];
    q.s = source_of(f);
    q.v = view_of(f);
  } else {
    Src& s = q.s;
    View& v = q.v;
    s.p0 = imgs + (size_t)b * H * W * 3; s.p1 = nullptr;
    s.pitch0 = 3 * W; s.pitch1 = 0; s.nv12 = 0; s.bpp = 3; s.ro = 0;
    s.cvr = s.cug = s.cvg = s.cub = 0;
    v.rot = 0; v.sw = W; v.sh = H; v.wt1 = v.ht1 = 0.f;
    v.ax = v.ay = 1.f; v.bx = v.by = 0.f;                             // f = p * 1 + 0 = p exactly
  }
  return q;
}

// the four taps of one sample as RGB (step 5 of the rule)
struct Quad { int r00, g00, b00, r01, g01, b01, r10, g10, b10, r11, g11, b11; };
__device__ __forceinline__ Quad quad_of(const Slot& q, const G6dFrame* __restrict__ frames, int r, const Taps& t) {
  const Src& s = q.s;
  Quad p;
  if (q.ext) {                                                        // every tap is taken, as below: a weight-0 tap is clamped inside the source
    Tap t00, t01, t10, t11;
    ext_taps<false>(yuv_of(frames[r]), t.x0, t.x1, t.y0, t.y1, true, true, t00, t01, t10, t11);
    p.r00 = t00.r; p.g00 = t00.g; p.b00 = t00.b; p.r01 = t01.r; p.g01 = t01.g; p.b01 = t01.b;
    p.r10 = t10.r; p.g10 = t10.g; p.b10 = t10.b; p.r11 = t11.r; p.g11 = t11.g; p.b11 = t11.b;
  } else if (s.nv12) {                                                // (block-uniform) a UV sample is loaded once for the taps that share it
    const bool sx = (t.x1 >> 1) == (t.x0 >> 1), sy = (t.y1 >> 1) == (t.y0 >> 1);
    const Chroma k00 = chroma(s, t.x0 >> 1, t.y0 >> 1);
    const Chroma k01 = sx ? k00 : chroma(s, t.x1 >> 1, t.y0 >> 1);
    const Chroma k10 = sy ? k00 : chroma(s, t.x0 >> 1, t.y1 >> 1);
    const Chroma k11 = sx ? k10 : (sy ? k01 : chroma(s, t.x1 >> 1, t.y1 >> 1));
    tap_nv12(s, k00, t.x0, t.y0, p.r00, p.g00, p.b00); tap_nv12(s, k01, t.x1, t.y0, p.r01, p.g01, p.b01);
    tap_nv12(s, k10, t.x0, t.y1, p.r10, p.g10, p.b10); tap_nv12(s, k11, t.x1, t.y1, p.r11, p.g11, p.b11);
  } else {
    tap_packed(s, t.x0, t.y0, p.r00, p.g00, p.b00); tap_packed(s, t.x1, t.y0, p.r01, p.g01, p.b01);
    tap_packed(s, t.x0, t.y1, p.r10, p.g10, p.b10); tap_packed(s, t.x1, t.y1, p.r11, p.g11, p.b11);
  }
  return p;
}

__device__ __forceinline__ int samples_of(const float* __restrict__ h, int dh, int dw, const View& v, int max_n) {
  const float cx = 0.5f * (float)(dw - 1), cy = 0.5f * (float)(dh - 1);
  const float2 p = pos_of(h, cx, cy, v), px = pos_of(h, cx + 1.f, cy, v), py = pos_of(h, cx, cy + 1.f, v);
  const float m = fmaxf(hypotf(px.x - p.x, px.y - p.y), hypotf(py.x - p.x, py.y - p.y));
  // a NaN fails both comparisons and an infinite length the second: a degenerate map of a parked slot takes one sample, and the cap is
  // applied before the conversion, so no float outside int's range is converted
  if (!(m >= 1.5f) || !(m <= 3.4028234e38f)) return 1;
  return (int)fminf(floorf(m + 0.5f), (float)max_n);
}

__global__ void __launch_bounds__(256) frame_crop_area_kernel(const G6dFrame* __restrict__ frames, const int* __restrict__ rec,
                                                             const unsigned char* __restrict__ imgs, int H, int W,
                                                             const float* __restrict__ hinv, float* __restrict__ dst, int dh, int dw, int tiles_x,
                                                             int max_n) {
  const int b = blockIdx.y;
  const int x = (blockIdx.x % tiles_x) * CW + (threadIdx.x & (CW - 1)), y = (blockIdx.x / tiles_x) * CH + threadIdx.x / CW;
  const int r = rec[b];
  const Slot q = slot_of(frames, r, imgs, b, H, W);
  const float* h = hinv + 9 * b;
  const int n = samples_of(h, dh, dw, q.v, max_n);
  if (x >= dw || y >= dh) return;
  const float step = 1.f / (float)(2 * n), mean = 1.f / (float)(n * n);   // n = 1: offsets 0, mean 1
  float ar = 0.f, ag = 0.f, ab = 0.f;
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    const float ys = (float)y + (float)(2 * j + 1 - n) * step;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
      const Taps t = taps_of(h, (float)x + (float)(2 * i + 1 - n) * step, ys, q.v);
      const Quad p = quad_of(q, frames, r, t);
      ar += weighted(t, p.r00, p.r01, p.r10, p.r11);
      ag += weighted(t, p.g00, p.g01, p.g10, p.g11);
      ab += weighted(t, p.b00, p.b01, p.b10, p.b11);
    }
  }
  const size_t plane = (size_t)dh * dw;
  float* o = dst + (size_t)b * 3 * plane + (size_t)y * dw + x;
  o[0] = level(ar * mean);
  o[plane] = level(ag * mean);
  o[2 * plane] = level(ab * mean);
}

}  // namespace

extern "C" int g6d_frame_crop(const G6dFrame* frames, const int32_t* rec, const uint8_t* imgs, int B, int H, int W, const float* hinv,
                              float* dst, int dh, int dw, g6d_stream_t stream) {
  if (!frames || !rec || !imgs || !hinv || !dst || B < 1 || B > 65535 || H < 1 || W < 1 || dh < 1 || dw < 1) {
    g6d_set_error("frame_crop: bad args (null table / rec / imgs / hinv / dst, B outside 1..65535, a non-positive canvas or crop)");
    return G6D_EINVAL;
  }
  const int tiles_x = (int)(((long long)dw + CW - 1) / CW);
  const long long tiles = (long long)tiles_x * (((long long)dh + CH - 1) / CH);
  if ((long long)dw + CW - 1 > 0x7fffffffLL || (long long)dh + CH - 1 > 0x7fffffffLL || tiles > 0x7fffffffLL) { g6d_set_error("frame_crop: too many tiles for one launch"); return G6D_EINVAL; }
  hipLaunchKernelGGL(frame_crop_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frames, rec,
                     imgs, H, W, hinv, dst, dh, dw, tiles_x);
  return g6d_check_launch("frame_crop");
}

extern "C" int g6d_frame_crop_area(const G6dFrame* frames, const int32_t* rec, const uint8_t* imgs, int B, int H, int W, const float* hinv,
                                   float* dst, int dh, int dw, int max_n, g6d_stream_t stream) {
  if (!frames || !rec || !imgs || !hinv || !dst || B < 1 || B > 65535 || H < 1 || W < 1 || dh < 1 || dw < 1 || max_n < 1 || max_n > 8) {
    g6d_set_error("frame_crop_area: bad args (null table / rec / imgs / hinv / dst, B outside 1..65535, a non-positive canvas or crop, "
                  "max_n outside 1..8)");
    return G6D_EINVAL;
  }
  const int tiles_x = (int)(((long long)dw + CW - 1) / CW);
  const long long tiles = (long long)tiles_x * (((long long)dh + CH - 1) / CH);
  if ((long long)dw + CW - 1 > 0x7fffffffLL || (long long)dh + CH - 1 > 0x7fffffffLL || tiles > 0x7fffffffLL) { g6d_set_error("frame_crop_area: too many tiles for one launch"); return G6D_EINVAL; }
  hipLaunchKernelGGL(frame_crop_area_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frames,
                     rec, imgs, H, W, hinv, dst, dh, dw, tiles_x, max_n);
  return g6d_check_launch("frame_crop_area");
}
