// One tap of a camera-native frame (G6dFrame, include/gen6d_hip.h) -> RGB by the ingest's tap rules: packed formats through `ro`, `bpp` and
// the row pitch, NV12 through the header's integer conversion with chroma UV[y>>1][x>>1].  Shared by the kernels that read source pictures
// (ingest.hip, frame_crop.hip).
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

}  // namespace
