// The host-side part that the float multi-map entry points share (G6dWinoSeg / G6dCorrSeg tables, include/gen6d_hip.h): validate every
// segment, find the lowest address of each kind, turn the segments into 32-bit float offsets from those bases, and refuse tables that
// reach beyond what the kernel can address.  Host code only; the per-entry argument checks stay at the entry points.
#pragma once
#include <stdio.h>
#include "g6d_common.h"

constexpr int G6D_MAX_SEG = 4;
// How far (in floats) a launch reaches from its lowest input address
constexpr long long G6D_REACH_BUFFER_LOAD = 1ll << 29;      // 2 GB: the bound of the buffer loads (wino_conv.hip, wino16_conv.hip, wino43_conv.hip)
constexpr long long G6D_REACH_CORR_PATCH = 1ll << 30;       // the bound of corr_patch.hip's addressing
constexpr long long G6D_REACH_OUT = 1ll << 31;              // outputs: 32-bit float offsets
// Hints of the bad-row message: tables that may give full outputs, pooled outputs or both; the Winograd correlations' rule on row lengths
#define G6D_SAME_KINDS " (all segments give the same kinds of output)"
#define G6D_SHARED_LD_IN " (all maps share ld_in)"

// One segment of either table type: a G6dCorrSeg has one kind of output, which it must give (the "full" one here)
struct G6dSeg {
  const float* in; float* full; float* pool;
  int N, H, W, ld_in, ld_full, ld_pool;
  int in_off, full_off, pool_off;      // floats from G6dSegTable's bases (filled by g6d_seg_table)
};
static inline G6dSeg g6d_seg(const G6dWinoSeg& g) { return G6dSeg{g.in, g.out_full, g.out_pool, g.N, g.H, g.W, g.ld_in, g.ld_full, g.ld_pool, 0, 0, 0}; }
static inline G6dSeg g6d_seg(const G6dCorrSeg& g) { return G6dSeg{g.in, g.out, nullptr, g.N, g.H, g.W, g.ld_in, g.ld_out, 0, 0, 0, 0}; }
static inline bool g6d_gives_full(const G6dWinoSeg& g) { return g.out_full != nullptr; }
static inline bool g6d_gives_full(const G6dCorrSeg&) { return true; }

struct G6dSegTable {
  const float* in; float* full; float* pool;      // common bases: the lowest address of each kind
  int nseg;
  G6dSeg seg[G6D_MAX_SEG];
};

// "<entry>: bad <noun><hint>" -> G6D_EINVAL
static inline int g6d_bad_seg(const char* entry, const char* noun, const char* hint) {
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: bad %s%s", entry, noun, hint);
  g6d_set_error(msg);
  return G6D_EINVAL;
}

// segs[0..nseg) (1 <= nseg <= G6D_MAX_SEG, checked by the caller) -> t, or G6D_EINVAL with the cause in g6d_last_error().  entry: the
// entry point's name in messages; noun: what it calls a table row ("segment" / "map"); hint: appended to the bad-row message;
// in_reach: G6D_REACH_BUFFER_LOAD or G6D_REACH_CORR_PATCH, a power of two.
template <class Seg>
int g6d_seg_table(const char* entry, const char* noun, const char* hint, const Seg* segs, int nseg, int Cin, int Cout, long long in_reach,
                  G6dSegTable& t) {
  char msg[200];
  const bool want_full = g6d_gives_full(segs[0]), want_pool = g6d_seg(segs[0]).pool != nullptr;
  if (!want_full && !want_pool) { snprintf(msg, sizeof(msg), "%s: no output", entry); g6d_set_error(msg); return G6D_EINVAL; }
  t.in = segs[0].in; t.full = g6d_seg(segs[0]).full; t.pool = g6d_seg(segs[0]).pool; t.nseg = nseg;
  for (int k = 0; k < nseg; ++k) {
    const G6dSeg g = g6d_seg(segs[k]);
    if (!g.in || (g.full != nullptr) != want_full || (g.pool != nullptr) != want_pool || g.N <= 0 || g.H <= 0 || g.W <= 0 || (g.ld_in & 3) ||
        g.ld_in < Cin || (want_full && g.ld_full < Cout) || (want_pool && (g.ld_pool < Cout || g.H < 2 || g.W < 2)) || !g6d_aligned16(g.in))
      return g6d_bad_seg(entry, noun, hint);
    if (g.in < t.in) t.in = g.in;
    if (want_full && g.full < t.full) t.full = g.full;
    if (want_pool && g.pool < t.pool) t.pool = g.pool;
    t.seg[k] = g;
  }
  // the kernels address with 32-bit float offsets from the common bases
  for (int k = 0; k < nseg; ++k) {
    G6dSeg& g = t.seg[k];
    const long long io = g.in - t.in, fo = want_full ? g.full - t.full : 0, po = want_pool ? g.pool - t.pool : 0;
    const long long px = (long long)g.N * g.H * g.W;
    if (io + px * g.ld_in >= in_reach || fo + px * g.ld_full >= G6D_REACH_OUT || po + px * g.ld_pool >= G6D_REACH_OUT) {
      int log2 = 0;
      while ((1ll << log2) < in_reach) ++log2;
      snprintf(msg, sizeof(msg), "%s: %ss must lie within 2^%d floats of each other (allocate them from one buffer)", entry, noun, log2);
      g6d_set_error(msg);
      return G6D_EINVAL;
    }
    g.in_off = (int)io; g.full_off = (int)fo; g.pool_off = (int)po;
  }
  return G6D_OK;
}
