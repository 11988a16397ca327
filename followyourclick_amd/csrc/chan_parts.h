// Row-tile partial channel sums (fyc_gemm chan_parts) folded by their consumer: shared by norm.hip and panel_linear.hip.
#pragma once
#include "fyc_common.h"

// {sum, sum of squares} of channel n over the statistics samples [o * group, (o + 1) * group) straight from the row-tile partials a
// producer's epilogue wrote (fyc_gemm chan_parts: [tile][slot][N][2] f32, slot sl of tile t = statistics sample (t * tile_rows) / cs_rows
// + sl): what fyc_chan_stats_reduce computes for output sample o - the same tile range, slot -> sample mapping and clamp at the last
// tile - for a consumer that folds the partials in its own prologue.  Fixed order (tiles ascending, slots ascending, f64): bitwise
// repeatable.  rows = all rows of the producer's output (< 2^31: 32-bit index math, a 64-bit division per tile costs more than the loads).
struct ChanParts { const float* parts; int tile_rows, slots, cs_rows, rows; };

// the tiles [t0, t1] that overlap output sample o and its statistics samples [lo, hi): the same for every channel, computed once per block
struct ChanPartsRange { int t0, t1, lo, hi, nsamp; };
__device__ __forceinline__ ChanPartsRange chan_parts_range(const ChanParts& cp, int o, int group) {
  ChanPartsRange r;
  const unsigned row0 = (unsigned)o * (unsigned)group * (unsigned)cp.cs_rows, row1 = row0 + (unsigned)group * (unsigned)cp.cs_rows;
  const int tiles_m = (int)(((unsigned)cp.rows + (unsigned)cp.tile_rows - 1u) / (unsigned)cp.tile_rows);
  r.nsamp = (int)((unsigned)cp.rows / (unsigned)cp.cs_rows);
  r.t0 = (int)(row0 / (unsigned)cp.tile_rows);
  r.t1 = (int)((row1 - 1u) / (unsigned)cp.tile_rows);
  if (r.t1 >= tiles_m) r.t1 = tiles_m - 1;
  r.lo = o * group;
  r.hi = (o + 1) * group;
  return r;
}

__device__ __forceinline__ void fold_chan_parts(const ChanParts& cp, const ChanPartsRange& r, int N, int n, double& s, double& q) {
  s = 0.0; q = 0.0;
  const float2* base = reinterpret_cast<const float2*>(cp.parts) + n;
  if (cp.slots == 1 && (unsigned)cp.cs_rows % (unsigned)cp.tile_rows == 0) {
    // whole tiles per sample: four loads in flight, added in tile order
    const unsigned per = (unsigned)cp.cs_rows / (unsigned)cp.tile_rows;     // tiles per statistics sample (>= 1)
    int t = r.t0;
    for (; t + 3 <= r.t1; t += 4) {
      float2 v[4];
      bool ok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = (int)((unsigned)(t + i) / per);
        ok[i] = f >= r.lo && f < r.hi && f < r.nsamp;
        v[i] = ok[i] ? base[(size_t)(t + i) * N] : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (ok[i]) { s += (double)v[i].x; q += (double)v[i].y; }
    }
    for (; t <= r.t1; ++t) {
      const int f = (int)((unsigned)t / per);
      if (f < r.lo || f >= r.hi || f >= r.nsamp) continue;
      const float2 v = base[(size_t)t * N];
      s += (double)v.x; q += (double)v.y;
    }
    return;
  }
  for (int t = r.t0; t <= r.t1; ++t) {
    const int first = (int)(((unsigned)t * (unsigned)cp.tile_rows) / (unsigned)cp.cs_rows);
    float2 v[4];
    bool ok[4];
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {                 // (at most 4 slots: EngineBase._cs_plan, fyc_gemm_stat_layout)
      const int f = first + sl;
      ok[sl] = sl < cp.slots && f >= r.lo && f < r.hi && f < r.nsamp;
      v[sl] = ok[sl] ? base[((size_t)t * cp.slots + sl) * N] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int sl = 0; sl < 4; ++sl)
      if (ok[sl]) { s += (double)v[sl].x; q += (double)v[sl].y; }
  }
}
