// gridscan.h - the building blocks the index builders share (knn.hip, mesh.hip, fields.hip, bookkeeping.hip), each ONCE:
//
//   grid fit     hgs_grid_volume / hgs_grid_fit: the uniform grid of a bounding box - flat axes thickened, the cell edge
//                grown until the grid fits its cell budget; hgs_grid_cell1: the cell of a coordinate
//   float keys   hgs_float_key / hgs_key_float: unsigned images of floats with the same order (atomicMin / atomicMax)
//   box          hgs_box_reduce: wave min / max of the points a lane takes, one atomic per wave, axis and bound
//   scan         hgs_scan_totals -> hgs_scan_carry -> hgs_scan_prefix: the device-wide exclusive scan over 1024-element
//                blocks, for uint32_t, for the uint2 pair marching cubes scans and for double (the surface sampler's
//                table of face areas: sums in element order)
//
// The grid fit and the cell index are plain C++ (no HIP types), like cellmask.h: the SAME functions are compiled into the
// kernels and into the host-side checker tests/gridfit_host.cpp.  cbrtf stays with the callers (their first cell edge h0),
// so what is here is exactly reproducible on the host: + - * / floorf fminf fmaxf, built with -ffp-contract=off.
#pragma once
#include "cellmask.h"   // HGS_HD, <math.h>, <stdint.h>

#define HGS_GRID_AXIS_MAX 4096         // cells per axis
#define HGS_SCAN_BLOCK 1024u           // elements per scan block = threads of a scan workgroup

// ---- grid fit ------------------------------------------------------------------------------------------------------
// Volume of a box of extents ext (emax = the longest, > 0): flat axes (a planar or collinear cloud) count with 1e-3 of the
// longest instead of 0.  The callers derive their first cell edge from it (knn: cbrtf(2 vol / P), mesh: cbrtf(vol / 8F)).
HGS_HD float hgs_grid_volume(const float ext[3], float emax) {
  const float floor_ext = emax * 1e-3f;
  return fmaxf(ext[0], floor_ext) * fmaxf(ext[1], floor_ext) * fmaxf(ext[2], floor_ext);
}

// Cells per axis g of a grid of cell edge >= h0 over the box: h grows by 1.26 (a doubling of the cell volume) for up to 64
// rounds, until the grid has at most nc_max cells and fewer than HGS_GRID_AXIS_MAX per axis.  Returns h.  (64 rounds
// always suffice for finite extents; a caller that cannot rely on it checks g[0] * g[1] * g[2] <= nc_max itself.)
HGS_HD float hgs_grid_fit(const float ext[3], float h0, uint32_t nc_max, uint32_t g[3]) {
  float h = h0;
  for (int it = 0; it < 64; ++it) {
    unsigned long long n = 1;
    for (int a = 0; a < 3; ++a) {
      const float c = floorf(ext[a] / h) + 1.0f;
      g[a] = c < 1.0f ? 1u : (c > (float)HGS_GRID_AXIS_MAX ? (uint32_t)HGS_GRID_AXIS_MAX : (uint32_t)c);
      n *= g[a];
    }
    const float lim = (float)(HGS_GRID_AXIS_MAX - 1);
    if (n <= nc_max && ext[0] / h < lim && ext[1] / h < lim && ext[2] / h < lim) break;
    h *= 1.26f;
  }
  return h;
}

// Cell of coordinate x on an axis of g cells from `origin`, clamped into the grid (NaN -> 0: fmaxf drops it).  The same
// fp32 operations wherever a cell is computed: when a grid is planned, built and searched.
HGS_HD int hgs_grid_cell1(float x, float origin, float inv_h, int g) {
  return (int)fminf(fmaxf(floorf((x - origin) * inv_h), 0.0f), (float)(g - 1));
}

#ifdef __HIPCC__
// ---- ordered float keys ------------------------------------------------------------------------------------------------
// float <-> unsigned key with the same order (atomicMin / atomicMax on floats of any sign).  An empty box is
// bmin = all ones, bmax = 0 (api.hip::box_init).
__device__ __forceinline__ uint32_t hgs_float_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float hgs_key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- box reduction -------------------------------------------------------------------------------------------------
// Every lane of the wave calls it (no early return in front); lanes with `take` contribute their point.  Wave max / min
// on the keys (DPP), then lane 0 issues one ordered-integer atomic per axis and bound - none for a wave that took nothing.
__device__ __forceinline__ void hgs_box_reduce(bool take, float x, float y, float z, uint32_t* __restrict__ bmin,
                                               uint32_t* __restrict__ bmax) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (take) { lo[0] = hi[0] = hgs_float_key(x); lo[1] = hi[1] = hgs_float_key(y); lo[2] = hi[2] = hgs_float_key(z); }
  const bool any = __ballot(take) != 0ull;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    hi[a] = hgs_wave_max_u32(hi[a]);
    lo[a] = ~hgs_wave_max_u32(~lo[a]);
  }
  if ((threadIdx.x & 63) == 0 && any) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(&bmin[a], lo[a]); atomicMax(&bmax[a], hi[a]); }
  }
}

// ---- device-wide exclusive scan ------------------------------------------------------------------------------------------
// Three launches of HGS_SCAN_BLOCK threads over v[0 .. n), T = uint32_t, uint2 (both components at once) or double:
//   1  hgs_scan_totals   ceil(n / 1024) workgroups: bsum[block] = the block's total
//   2  hgs_scan_carry    ONE workgroup: bsum -> exclusive, 1024 totals a round with the carry in a register; returns the
//                        grand total to every thread (also the whole scan of a short array: hgs_k_field_order)
//   3  hgs_scan_prefix   ceil(n / 1024) workgroups: every thread gets its element's index, exclusive prefix and raw value
// bsum holds ceil(n / 1024) elements (api.hip::scan_shape).  The kernels around them supply n and their epilogue.
__device__ __forceinline__ uint32_t hgs_scan_1k(uint32_t v, uint32_t* wtot, uint32_t& tot) {
  return hgs_block_excl_scan<HGS_SCAN_BLOCK>(v, wtot, tot);
}
__device__ __forceinline__ uint2 hgs_scan_1k(uint2 v, uint32_t* wtot, uint2& tot) {
  const uint32_t ex = hgs_block_excl_scan<HGS_SCAN_BLOCK>(v.x, wtot, tot.x);
  const uint32_t ey = hgs_block_excl_scan<HGS_SCAN_BLOCK>(v.y, wtot, tot.y);
  return make_uint2(ex, ey);
}

// T = double (surface.hip: the table of face areas): the workgroup's prefixes are the LEFT-TO-RIGHT sums
// ((v0 + v1) + v2) + ..., element by element - the waves take turns, each continues the sum where the wave in front left
// it.  That order is what makes a table of non-negative addends usable as it stands: the prefixes never decrease, and
// a zero addend repeats the prefix in front of it bit for bit.  (A tree of partial sums promises neither.)  1024 dependent
// additions per workgroup, some microseconds: for tables built once, not for a hot path.
__device__ __forceinline__ double hgs_scan_1k(double v, double* wtot, double& tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int vlo = __double2loint(v), vhi = __double2hiint(v);
  double ex = 0.0;
  __syncthreads();                 // protect wtot from a previous use
  for (int r = 0; r < (int)(HGS_SCAN_BLOCK / 64); ++r) {
    if (w == r) {
      double run = r ? wtot[r - 1] : 0.0;
#pragma unroll 4                   // (all 64 at once keep 128 lane values in scalar registers and spill)
      for (int k = 0; k < 64; ++k) {
        if (lane == k) ex = run;
        run += __hiloint2double(__builtin_amdgcn_readlane(vhi, k), __builtin_amdgcn_readlane(vlo, k));
      }
      if (lane == 0) wtot[r] = run;
    }
    __syncthreads();
  }
  tot = wtot[HGS_SCAN_BLOCK / 64 - 1];
  return ex;
}

// what a workgroup keeps in LDS per wave for the scan of T
template <class T> struct hgs_scan_lds { typedef uint32_t type; };
template <> struct hgs_scan_lds<double> { typedef double type; };

// element i of v[0 .. n) (zero behind the end) scanned over the workgroup: the exclusive prefix; raw = the element, tot =
// the workgroup's total
template <class T>
__device__ __forceinline__ T hgs_scan_block(const T* v, uint32_t i, uint32_t n, T& raw, T& tot) {
  __shared__ typename hgs_scan_lds<T>::type wtot[HGS_SCAN_BLOCK / 64];
  raw = i < n ? v[i] : T();
  return hgs_scan_1k(raw, wtot, tot);
}

template <class T>
__device__ __forceinline__ void hgs_scan_totals(uint32_t n, const T* v, T* bsum) {
  T raw, tot;
  hgs_scan_block(v, blockIdx.x * HGS_SCAN_BLOCK + threadIdx.x, n, raw, tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// out[0 .. nb) = exclusive scan of in[0 .. nb) (out may be in); returns the total.  No barrier closes a round: the one
// hgs_block_excl_scan OPENS with has to stay - it protects wtot from the round before and orders a caller's LDS work in
// front of this call (the class histogram of hgs_k_field_order) before what follows it.
template <class T>
__device__ __forceinline__ T hgs_scan_carry(uint32_t nb, const T* in, T* out) {
  T carry = T();
  for (uint32_t b0 = 0; b0 < nb; b0 += HGS_SCAN_BLOCK) {
    const uint32_t b = b0 + threadIdx.x;
    T raw, tot;
    const T ex = hgs_scan_block(in, b, nb, raw, tot);
    if (b < nb) out[b] = carry + ex;
    carry += tot;
  }
  return carry;
}

// true for a live element (i < n); ex = its exclusive prefix over the whole array; raw = its value (zero where not live)
template <class T>
__device__ __forceinline__ bool hgs_scan_prefix(uint32_t n, const T* v, const T* bsum, uint32_t& i, T& ex, T& raw) {
  T tot;
  i = blockIdx.x * HGS_SCAN_BLOCK + threadIdx.x;
  ex = hgs_scan_block(v, i, n, raw, tot) + bsum[blockIdx.x];
  return i < n;
}
#endif  // __HIPCC__
