// fields.hip - the density field of the Gaussians on a regular grid and its iso-surface (include/hgs_rast.h: hgs_field_*,
// hgs_mc_*; the reference's GaussianModel.extract_fields + mcubes.marching_cubes).  Included by api.hip - one translation
// unit, under the no-scratch rule of tests/test_kernel_resources_cpu.py.  Box reduction and scans: gridscan.h.
//
// Field:  bbox -> setup -> gauss (record + reached block range per Gaussian) -> lists(count)      [hgs_field_plan]
//         order (scan of the counts, blocks heaviest first) -> lists(fill) -> eval                  [hgs_field_eval]
// A block's list is filled by ONE wave that walks the Gaussians' 4-byte block ranges in index order and compacts the hits
// (ballot + prefix count): ascending Gaussian index by construction, no atomics, so the sum order of the evaluation - and
// with it every bit of the field - is the same in every call.  The walk reads P * 4 B per non-empty block out of L2; the
// evaluation does 512 exp2 per listed Gaussian and dominates it.
//
// Marching cubes:  count (crossing mask per grid point, triangles per cell) -> scan1/2/3 -> emit (vertices per crossed edge,
// triangles per cell through the edge -> vertex map).
//
// Point samples (hgs_fsample: density, normal and colour at arbitrary points, over the lists hgs_field_eval left):
//         bin (block per point, points per block) -> table (scan of points and of runs of 256) -> scatter -> eval
#pragma once
#include "hgs_common.h"

#define HGS_MC_TABLE_QUAL __constant__ static const
#include "mc_table.h"

#define HGS_FIELD_MAX_BLOCKS 32          // per axis: a block range is 2 x 5 bits per axis
#define HGS_FIELD_MAX_RES 2048
#define HGS_FIELD_MAX_SPLIT 256         // samples per block and axis: a block's work items (split^3 / 2) stay far inside 32 bits
#define HGS_FIELD_REC_FLOATS 10          // centre, six folded coefficients, opacity
#define HGS_FIELD_CHUNK 256              // records staged through LDS at a time
#define HGS_FIELD_LDS_F4 3               // a staged record: 3 x float4 (48 B, ds_read_b128 broadcasts)
#define HGS_FIELD_NONE 0xffffffffu       // reach of a Gaussian that is in no list
#define HGS_FIELD_OPACITY_CUT 0.005f

struct FieldPlanPtrs {
  float2* rec;          // [P][5]
  uint32_t* reach;      // [P]  lo / hi block per axis, 5 bits each (x lo, x hi, y lo, ...), or HGS_FIELD_NONE
  float* bounds;        // [2][HGS_FIELD_MAX_BLOCKS]: lo_b, hi_b
  uint32_t* counts;     // [nb^3]
};
struct FieldListPtrs {
  uint32_t* start;      // [nb^3 + 1]
  uint32_t* order;      // [nb^3] blocks, longest list first
  uint32_t* refs;       // [num_refs] Gaussian indices, block by block, ascending inside a block
};
struct FieldDims { int32_t P, R, nb, split; };

__device__ __forceinline__ bool field_kept(int i, const float* __restrict__ xyz, const float* __restrict__ opacity, float3& p) {
  p = make_float3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
  return opacity[i] > HGS_FIELD_OPACITY_CUT && isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_field_bbox(int P, const float* __restrict__ xyz, const float* __restrict__ opacity, hgs_field_info* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float3 p = make_float3(0.f, 0.f, 0.f);
  const bool kept = i < P && field_kept(i, xyz, opacity, p);
  hgs_box_reduce(kept, p.x, p.y, p.z, info->bmin, info->bmax);
  const uint32_t n = (uint32_t)__popcll(__ballot(kept));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&info->num_kept, n);
}

// one workgroup: centre, extent and scale from the box; the blocks' bounds from the axis
extern "C" __global__ void __launch_bounds__(64)
hgs_k_field_setup(FieldDims D, const float* __restrict__ axis, float grow, FieldPlanPtrs pp, hgs_field_info* __restrict__ info) {
  const int t = threadIdx.x;
  if (t < D.nb) {
    pp.bounds[t] = axis[t * D.split] - grow;
    pp.bounds[HGS_FIELD_MAX_BLOCKS + t] = axis[t * D.split + D.split - 1] + grow;
  }
  if (t != 0) return;
  float ext = 0.0f;
  for (int a = 0; a < 3; ++a) {
    const float mn = info->num_kept ? hgs_key_float(info->bmin[a]) : 0.0f, mx = info->num_kept ? hgs_key_float(info->bmax[a]) : 0.0f;
    info->center[a] = (mn + mx) / 2.0f;
    ext = fmaxf(ext, mx - mn);
  }
  info->extent = ext;
  info->scale = (float)(1.8 / (double)ext);
  info->num_gaussians = D.P;
  info->num_blocks = D.nb;
  info->resolution = D.R;
  info->grow = grow;
}

// per Gaussian: the staged record and the range of blocks that list it
extern "C" __global__ void __launch_bounds__(256)
hgs_k_field_gauss(FieldDims D, const float* __restrict__ xyz, const float* __restrict__ opacity,
                  const float* __restrict__ scaling, const float* __restrict__ rotation, FieldPlanPtrs pp,
                  const hgs_field_info* __restrict__ info) {
  __shared__ float bnd[2 * HGS_FIELD_MAX_BLOCKS];
  if ((int)threadIdx.x < D.nb) {                            // (only the first nb of each half are written by the setup)
    bnd[threadIdx.x] = pp.bounds[threadIdx.x];
    bnd[HGS_FIELD_MAX_BLOCKS + threadIdx.x] = pp.bounds[HGS_FIELD_MAX_BLOCKS + threadIdx.x];
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.P) return;
  float3 p;
  uint32_t reach = HGS_FIELD_NONE;
  if (field_kept(i, xyz, opacity, p)) {
    const float sc = info->scale;
    const float n[3] = {(p.x - info->center[0]) * sc, (p.y - info->center[1]) * sc, (p.z - info->center[2]) * sc};
    uint32_t r = 0;
    bool any = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int lo = HGS_FIELD_MAX_BLOCKS, hi = -1;
      for (int b = 0; b < D.nb; ++b)
        if (n[a] > bnd[b] && n[a] < bnd[HGS_FIELD_MAX_BLOCKS + b]) { lo = min(lo, b); hi = b; }
      any = any && hi >= 0;
      r |= ((uint32_t)(lo & 31) | ((uint32_t)(hi & 31) << 5)) << (10 * a);
    }
    if (any) reach = r;
    // Sigma^-1 = R diag(1 / s^2) R^T, folded for exp2: p2 = log2(e) * power = A dx^2 + D dy^2 + F dz^2 + B dx dy + C dx dz + E dy dz
    float qr = rotation[4 * (size_t)i], qx = rotation[4 * (size_t)i + 1], qy = rotation[4 * (size_t)i + 2], qz = rotation[4 * (size_t)i + 3];
    const float qn = 1.0f / sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
    qr *= qn; qx *= qn; qy *= qn; qz *= qn;
    const float Rm[3][3] = {{1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qr * qz), 2.0f * (qx * qz + qr * qy)},
                            {2.0f * (qx * qy + qr * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qr * qx)},
                            {2.0f * (qx * qz - qr * qy), 2.0f * (qy * qz + qr * qx), 1.0f - 2.0f * (qx * qx + qy * qy)}};
    float w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float s = scaling[3 * (size_t)i + k] * sc;
      w[k] = 1.0f / (s * s);
    }
    auto inv = [&](int r0, int r1) { return (Rm[r0][0] * Rm[r1][0] * w[0] + Rm[r0][1] * Rm[r1][1] * w[1]) + Rm[r0][2] * Rm[r1][2] * w[2]; };
    const float h = -0.5f * HGS_LOG2E, f = -HGS_LOG2E;
    float2* rec = pp.rec + (size_t)i * (HGS_FIELD_REC_FLOATS / 2);
    rec[0] = make_float2(n[0], n[1]);
    rec[1] = make_float2(n[2], h * inv(0, 0));            // A
    rec[2] = make_float2(f * inv(0, 1), f * inv(0, 2));   // B, C
    rec[3] = make_float2(h * inv(1, 1), f * inv(1, 2));   // D, E
    rec[4] = make_float2(h * inv(2, 2), opacity[i]);      // F, opacity
  }
  pp.reach[i] = reach;
}

__device__ __forceinline__ bool field_reaches(uint32_t r, uint32_t bx, uint32_t by, uint32_t bz) {
  // (HGS_FIELD_NONE: lo = 31 > hi... is not enough for block 31, hence the explicit test)
  return r != HGS_FIELD_NONE && bx >= (r & 31u) && bx <= ((r >> 5) & 31u) && by >= ((r >> 10) & 31u) && by <= ((r >> 15) & 31u) &&
         bz >= ((r >> 20) & 31u) && bz <= ((r >> 25) & 31u);
}

// One wave per block walks all reach words in index order.  fill == 0: counts[block] and the total; fill == 1: the list.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_field_lists(FieldDims D, FieldPlanPtrs pp, FieldListPtrs lp, int fill, hgs_field_info* __restrict__ info) {
  const uint32_t nblocks = (uint32_t)(D.nb * D.nb * D.nb);
  const uint32_t block = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (block >= nblocks) return;
  if (fill && pp.counts[block] == 0u) return;
  const uint32_t bz = block % (uint32_t)D.nb, by = (block / (uint32_t)D.nb) % (uint32_t)D.nb, bx = block / (uint32_t)(D.nb * D.nb);
  uint32_t* __restrict__ out = fill ? lp.refs + lp.start[block] : nullptr;
  uint32_t n = 0;
  for (int i0 = 0; i0 < D.P; i0 += 256) {
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i0 + 64 * k + (int)lane;
      r[k] = i < D.P ? pp.reach[i] : HGS_FIELD_NONE;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool hit = field_reaches(r[k], bx, by, bz);
      const unsigned long long m = __ballot(hit);
      if (fill && hit) out[n + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)(i0 + 64 * k) + lane;
      n += (uint32_t)__popcll(m);
    }
  }
  if (!fill && lane == 0) {
    pp.counts[block] = n;
    if (n) atomicAdd((unsigned long long*)&info->num_refs, (unsigned long long)n);
  }
}

// one workgroup: start[] = exclusive scan of the counts; order[] = the blocks by the bit length of their count, longest
// first (the evaluation's workgroups start in this order; where a block stands inside its class changes no result)
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_field_order(FieldDims D, FieldPlanPtrs pp, FieldListPtrs lp) {
  __shared__ uint32_t cls_n[33], cls_at[33];
  const uint32_t nblocks = (uint32_t)(D.nb * D.nb * D.nb);
  if (threadIdx.x < 33) cls_n[threadIdx.x] = 0u;
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nblocks; b += 1024u) atomicAdd(&cls_n[32 - __clz(pp.counts[b])], 1u);
  const uint32_t total = hgs_scan_carry(nblocks, pp.counts, lp.start);      // (its barriers also order the histogram)
  if (threadIdx.x == 0) {
    lp.start[nblocks] = total;
    uint32_t at = 0;
    for (int c = 32; c >= 0; --c) { cls_at[c] = at; at += cls_n[c]; }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nblocks; b += 1024u) lp.order[atomicAdd(&cls_at[32 - __clz(pp.counts[b])], 1u)] = b;
}

// The evaluation.  A workgroup takes one block (by the heavy-first order) or, where a block has more than 2 x 256 samples,
// one slab of it.  A thread owns the two samples (xp, y, z) and (xp + ceil(split / 2), y, z): they share dy and dz, so the
// y / z part of the quadratic form is computed once for both.  The block's records go through LDS 256 at a time; every
// lane reads the same record (a broadcast, 3 x ds_read_b128).
extern "C" __global__ void __launch_bounds__(256)
hgs_k_field_eval(FieldDims D, const float* __restrict__ axis, FieldPlanPtrs pp, FieldListPtrs lp, int slabs,
                 float* __restrict__ occ) {
  __shared__ float4 st[HGS_FIELD_CHUNK * HGS_FIELD_LDS_F4];
  const uint32_t block = lp.order[blockIdx.x / (uint32_t)slabs], slab = blockIdx.x % (uint32_t)slabs;
  const int s = D.split, half = (s + 1) / 2;
  const int items = half * s * s;
  const int j = (int)slab * (int)blockDim.x + (int)threadIdx.x;
  const bool live = j < items;
  const int jj = live ? j : 0;
  const int xp = jj / (s * s), y = (jj / s) % s, z = jj % s;
  const bool two = xp + half < s;
  const int bz = (int)(block % (uint32_t)D.nb), by = (int)((block / (uint32_t)D.nb) % (uint32_t)D.nb), bx = (int)(block / (uint32_t)(D.nb * D.nb));
  const int gx = bx * s + xp, gy = by * s + y, gz = bz * s + z;
  const float px0 = axis[gx], px1 = axis[two ? gx + half : gx], py = axis[gy], pz = axis[gz];
  const uint32_t first = lp.start[block], n = lp.start[block + 1] - first;
  float acc0 = 0.0f, acc1 = 0.0f;
  for (uint32_t c0 = 0; c0 < n; c0 += HGS_FIELD_CHUNK) {
    const uint32_t cn = min((uint32_t)HGS_FIELD_CHUNK, n - c0);
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < cn; r += blockDim.x) {
      const float2* __restrict__ rec = pp.rec + (size_t)lp.refs[first + c0 + r] * (HGS_FIELD_REC_FLOATS / 2);
      const float2 a = rec[0], b = rec[1], c = rec[2], d = rec[3], e = rec[4];
      st[r * HGS_FIELD_LDS_F4 + 0] = make_float4(a.x, a.y, b.x, b.y);     // nx ny nz A
      st[r * HGS_FIELD_LDS_F4 + 1] = make_float4(c.x, c.y, d.x, d.y);     // B C D E
      st[r * HGS_FIELD_LDS_F4 + 2] = make_float4(e.x, e.y, 0.0f, 0.0f);   // F opacity
    }
    __syncthreads();
    for (uint32_t r = 0; r < cn; ++r) {
      const float4 u = st[r * HGS_FIELD_LDS_F4 + 0], v = st[r * HGS_FIELD_LDS_F4 + 1], w = st[r * HGS_FIELD_LDS_F4 + 2];
      const float dy = py - u.y, dz = pz - u.z;
      const float q1 = __builtin_fmaf(v.x, dy, v.y * dz);                                   // B dy + C dz
      const float q0 = __builtin_fmaf(dy, __builtin_fmaf(v.z, dy, v.w * dz), (w.x * dz) * dz);   // D dy^2 + E dy dz + F dz^2
      const float dx0 = px0 - u.x, dx1 = px1 - u.x;
      const float p0 = __builtin_fmaf(dx0, __builtin_fmaf(u.w, dx0, q1), q0);
      const float p1 = __builtin_fmaf(dx1, __builtin_fmaf(u.w, dx1, q1), q0);
      const float e0 = p0 > 0.0f ? 0.0f : __builtin_amdgcn_exp2f(p0);
      const float e1 = p1 > 0.0f ? 0.0f : __builtin_amdgcn_exp2f(p1);
      acc0 = __builtin_fmaf(w.y, e0, acc0);
      acc1 = __builtin_fmaf(w.y, e1, acc1);
    }
  }
  if (live) {
    const size_t R = (size_t)D.R;
    occ[((size_t)gx * R + (size_t)gy) * R + (size_t)gz] = acc0;
    if (two) occ[((size_t)(gx + half) * R + (size_t)gy) * R + (size_t)gz] = acc1;
  }
}

// ------------------------------------------------------------------------------------------------ marching cubes

struct McDims { int32_t X, Y, Z; uint32_t N; };
struct McPtrs {
  uint2* offs;          // [N + 1] per grid point: (vertices, triangles) - counts, then exclusive offsets
  uint2* bsum;          // [ceil(N / 1024) + 1]
  uint8_t* mask;        // [N] bit a: the grid edge from the point along axis a is crossed
};
// cube edge -> low grid point of the edge (x | y << 1 | z << 2) | axis << 3, for the numbering of mc_table.h
__constant__ static const uint8_t HGS_MC_EDGE_AT[12] = {0, 9, 2, 8, 4, 13, 6, 12, 16, 17, 19, 18};

__device__ __forceinline__ bool mc_inside(float v, float thr) { return v >= thr; }

extern "C" __global__ void __launch_bounds__(256)
hgs_k_mc_count(McDims D, const float* __restrict__ f, float thr, McPtrs p) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= D.N) return;
  const int z = (int)(i % (uint32_t)D.Z), y = (int)((i / (uint32_t)D.Z) % (uint32_t)D.Y), x = (int)(i / (uint32_t)(D.Z * D.Y));
  const size_t sx = (size_t)D.Y * D.Z, sy = (size_t)D.Z;
  // a field with a dimension of one sample has no cell: no grid edge belongs to one, nothing is emitted (with two or more
  // samples on every axis each grid edge is an edge of at least one cell)
  const bool cells = D.X > 1 && D.Y > 1 && D.Z > 1;
  const bool hx = cells && x + 1 < D.X, hy = cells && y + 1 < D.Y, hz = cells && z + 1 < D.Z;
  const bool in0 = mc_inside(f[i], thr);
  uint32_t cse = in0 ? 1u : 0u, m = 0;
  if (hx) { const bool b = mc_inside(f[i + sx], thr); m |= (b != in0) ? 1u : 0u; cse |= b ? 2u : 0u; }
  if (hy) { const bool b = mc_inside(f[i + sy], thr); m |= (b != in0) ? 2u : 0u; cse |= b ? 8u : 0u; }
  if (hz) { const bool b = mc_inside(f[i + 1], thr); m |= (b != in0) ? 4u : 0u; cse |= b ? 16u : 0u; }
  uint32_t nt = 0;
  if (hx && hy && hz) {
    cse |= mc_inside(f[i + sx + sy], thr) ? 4u : 0u;
    cse |= mc_inside(f[i + sx + 1], thr) ? 32u : 0u;
    cse |= mc_inside(f[i + sx + sy + 1], thr) ? 64u : 0u;
    cse |= mc_inside(f[i + sy + 1], thr) ? 128u : 0u;
    for (int k = 0; k < HGS_MC_ROW - 1 && HGS_MC_TRI_TABLE[cse][k] >= 0; k += 3) ++nt;
  }
  p.mask[i] = (uint8_t)m;
  p.offs[i] = make_uint2((uint32_t)__popc(m), nt);
}

// exclusive scan of offs[0 .. N) in place, both components (gridscan.h on uint2); offs[N] and `info` receive the totals
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mc_scan1(McDims D, McPtrs p) { hgs_scan_totals(D.N, p.offs, p.bsum); }
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mc_scan2(McDims D, McPtrs p, hgs_mc_info* __restrict__ info) {
  const uint2 total = hgs_scan_carry((D.N + HGS_SCAN_BLOCK - 1u) / HGS_SCAN_BLOCK, p.bsum, p.bsum);
  if (threadIdx.x == 0) {
    p.offs[D.N] = total;
    info->num_vertices = total.x;
    info->num_triangles = total.y;
  }
}
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mc_scan3(McDims D, McPtrs p) {
  uint32_t i;
  uint2 ex, v;
  if (hgs_scan_prefix(D.N, p.offs, p.bsum, i, ex, v)) p.offs[i] = ex;
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_mc_emit(McDims D, const float* __restrict__ f, float thr, McPtrs p, uint32_t nv, uint32_t nt,
              float* __restrict__ vertices, int32_t* __restrict__ triangles) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= D.N) return;
  const int z = (int)(i % (uint32_t)D.Z), y = (int)((i / (uint32_t)D.Z) % (uint32_t)D.Y), x = (int)(i / (uint32_t)(D.Z * D.Y));
  const size_t sx = (size_t)D.Y * D.Z, sy = (size_t)D.Z;
  const uint2 at = p.offs[i], next = p.offs[i + 1];
  const uint32_t m = p.mask[i];
  if (m) {
    const float f0 = f[i];
    uint32_t k = at.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(m & (1u << a))) continue;
      const float f1 = f[i + (a == 0 ? sx : (a == 1 ? sy : (size_t)1))];
      const float t = fminf(fmaxf((thr - f0) / (f1 - f0), 0.0f), 1.0f);
      if (k < nv) {                                        // (always: the scan counted this edge)
        vertices[3 * (size_t)k] = (float)x + (a == 0 ? t : 0.0f);
        vertices[3 * (size_t)k + 1] = (float)y + (a == 1 ? t : 0.0f);
        vertices[3 * (size_t)k + 2] = (float)z + (a == 2 ? t : 0.0f);
      }
      ++k;
    }
  }
  if (next.y == at.y) return;                              // no triangle in this cell (or no cell at this point)
  uint32_t cse = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int cx = (c == 1 || c == 2 || c == 5 || c == 6), cy = (c == 2 || c == 3 || c == 6 || c == 7), cz = c >> 2;
    cse |= mc_inside(f[i + cx * sx + cy * sy + (size_t)cz], thr) ? (1u << c) : 0u;
  }
  uint32_t t = at.y;
  for (int k = 0; k < HGS_MC_ROW - 1 && HGS_MC_TRI_TABLE[cse][k] >= 0 && t < nt; k += 3, ++t) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint32_t e = HGS_MC_EDGE_AT[HGS_MC_TRI_TABLE[cse][k + c]];
      const size_t q = i + (e & 1u) * sx + ((e >> 1) & 1u) * sy + ((e >> 2) & 1u);
      const uint32_t axis = e >> 3;
      triangles[3 * (size_t)t + c] = (int32_t)(p.offs[q].x + (uint32_t)__popc(p.mask[q] & ((1u << axis) - 1u)));
    }
  }
}

// ------------------------------------------------------------------------------------------------ point samples

#define HGS_FSAMPLE_RUN 256              // points of one evaluation workgroup, one per thread
#define HGS_FSAMPLE_LDS_F4 4             // a staged record: the field's three float4 and the colour (64 B)

struct FSamplePtrs {
  uint32_t* blk;        // [M] block of the point, or HGS_FIELD_NONE (a coordinate that is not finite)
  uint32_t* cursor;     // [nb^3] zeroed; the scatter's position inside a bin
  uint2* tab;           // [nb^3 + 1] (points, runs) per block - counts (zeroed first), then exclusive offsets
  uint32_t* bins;       // [M] point indices, block by block
};
struct FSampleGeo { float cx, cy, cz, scale; int32_t normalized; };
struct FSampleOut { float* density; float* normal; float* color; };

__device__ __forceinline__ float3 fsample_normalised(const float* __restrict__ points, uint32_t i, const FSampleGeo& geo) {
  const float3 q = make_float3(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]);
  if (geo.normalized) return q;
  return make_float3((q.x - geo.cx) * geo.scale, (q.y - geo.cy) * geo.scale, (q.z - geo.cz) * geo.scale);
}

// (number of samples <= v) - 1, clamped to [0, R - 1]: the count runs over the samples 1 .. R - 1 (at most 11 steps)
__device__ __forceinline__ int fsample_cell(const float* __restrict__ axis, int R, float v) {
  int lo = 1, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (axis[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_fsample_bin(FieldDims D, uint32_t M, const float* __restrict__ points, const float* __restrict__ axis, FSampleGeo geo,
                  FSamplePtrs sp, FSampleOut out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= M) return;
  const float3 n = fsample_normalised(points, i, geo);
  if (!(isfinite(n.x) && isfinite(n.y) && isfinite(n.z))) {
    sp.blk[i] = HGS_FIELD_NONE;                            // no workgroup of the evaluation sees it: its zeros are written here
    if (out.density) out.density[i] = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (out.normal) out.normal[3 * (size_t)i + a] = 0.0f;
      if (out.color) out.color[3 * (size_t)i + a] = 0.0f;
    }
    return;
  }
  const uint32_t bx = (uint32_t)(fsample_cell(axis, D.R, n.x) / D.split), by = (uint32_t)(fsample_cell(axis, D.R, n.y) / D.split),
                 bz = (uint32_t)(fsample_cell(axis, D.R, n.z) / D.split);
  const uint32_t block = (bx * (uint32_t)D.nb + by) * (uint32_t)D.nb + bz;
  sp.blk[i] = block;
  atomicAdd(&sp.tab[block].x, 1u);
}

// one workgroup: tab[] = exclusive scan of (points, runs of HGS_FSAMPLE_RUN points) per block, the totals behind the end
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_fsample_table(FieldDims D, FSamplePtrs sp) {
  const uint32_t nblocks = (uint32_t)(D.nb * D.nb * D.nb);
  for (uint32_t b = threadIdx.x; b < nblocks; b += 1024u)          // (thread b % 1024 also scans element b)
    sp.tab[b].y = (sp.tab[b].x + (HGS_FSAMPLE_RUN - 1u)) / HGS_FSAMPLE_RUN;
  const uint2 total = hgs_scan_carry(nblocks, sp.tab, sp.tab);
  if (threadIdx.x == 0) sp.tab[nblocks] = total;
}

// where a point stands inside its bin changes no result: every point's sums are its own
extern "C" __global__ void __launch_bounds__(256)
hgs_k_fsample_scatter(uint32_t M, FSamplePtrs sp) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= M) return;
  const uint32_t block = sp.blk[i];
  if (block == HGS_FIELD_NONE) return;
  sp.bins[sp.tab[block].x + atomicAdd(&sp.cursor[block], 1u)] = i;
}

// A workgroup takes one run of a block's bin, a thread one point.  The launch has the host's upper bound of runs; the
// table says which (block, run) a workgroup is, and the surplus leaves.  The records go through LDS as in
// hgs_k_field_eval, with the colour in a fourth float4, and the power is spelled as there: a point on a grid sample gets
// the field's bits.  t = (2A dx + B dy + C dz, B dx + 2D dy + E dz, C dx + E dy + 2F dz) is the gradient of the folded
// form, so G = - sum of o e t.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_fsample_eval(FieldDims D, const float* __restrict__ points, const float* __restrict__ colors, FSampleGeo geo,
                   FieldPlanPtrs pp, FieldListPtrs lp, FSamplePtrs sp, FSampleOut out) {
  __shared__ float4 st[HGS_FIELD_CHUNK * HGS_FSAMPLE_LDS_F4];
  const uint32_t nblocks = (uint32_t)(D.nb * D.nb * D.nb);
  const uint32_t w = blockIdx.x;
  if (w >= sp.tab[nblocks].y) return;
  uint32_t lo = 0, hi = nblocks;                            // the last block whose first run is <= w (empty blocks in front of
  while (hi - lo > 1u) {                                    // it share its offset and are passed over)
    const uint32_t mid = (lo + hi) >> 1;
    if (sp.tab[mid].y <= w) lo = mid; else hi = mid;
  }
  const uint32_t block = lo;
  const uint2 at = sp.tab[block];
  const uint32_t j = (w - at.y) * HGS_FSAMPLE_RUN + threadIdx.x;
  const bool live = j < sp.tab[block + 1].x - at.x;
  const uint32_t i = live ? sp.bins[at.x + j] : 0u;
  float3 p = make_float3(0.0f, 0.0f, 0.0f);
  if (live) p = fsample_normalised(points, i, geo);
  const uint32_t first = lp.start[block], n = lp.start[block + 1] - first;
  float acc = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
  for (uint32_t c0 = 0; c0 < n; c0 += HGS_FIELD_CHUNK) {
    const uint32_t cn = min((uint32_t)HGS_FIELD_CHUNK, n - c0);
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < cn; r += blockDim.x) {
      const uint32_t g = lp.refs[first + c0 + r];
      const float2* __restrict__ rec = pp.rec + (size_t)g * (HGS_FIELD_REC_FLOATS / 2);
      const float2 a = rec[0], b = rec[1], c = rec[2], d = rec[3], e = rec[4];
      st[r * HGS_FSAMPLE_LDS_F4 + 0] = make_float4(a.x, a.y, b.x, b.y);     // nx ny nz A
      st[r * HGS_FSAMPLE_LDS_F4 + 1] = make_float4(c.x, c.y, d.x, d.y);     // B C D E
      st[r * HGS_FSAMPLE_LDS_F4 + 2] = make_float4(e.x, e.y, 0.0f, 0.0f);   // F opacity
      st[r * HGS_FSAMPLE_LDS_F4 + 3] = colors ? make_float4(colors[3 * (size_t)g], colors[3 * (size_t)g + 1], colors[3 * (size_t)g + 2], 0.0f)
                                              : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    for (uint32_t r = 0; r < cn; ++r) {
      const float4 u = st[r * HGS_FSAMPLE_LDS_F4 + 0], v = st[r * HGS_FSAMPLE_LDS_F4 + 1], k = st[r * HGS_FSAMPLE_LDS_F4 + 2],
                   col = st[r * HGS_FSAMPLE_LDS_F4 + 3];
      const float dy = p.y - u.y, dz = p.z - u.z;
      const float q1 = __builtin_fmaf(v.x, dy, v.y * dz);                                   // B dy + C dz
      const float q0 = __builtin_fmaf(dy, __builtin_fmaf(v.z, dy, v.w * dz), (k.x * dz) * dz);   // D dy^2 + E dy dz + F dz^2
      const float dx = p.x - u.x;
      const float pw = __builtin_fmaf(dx, __builtin_fmaf(u.w, dx, q1), q0);
      const float e = pw > 0.0f ? 0.0f : __builtin_amdgcn_exp2f(pw);
      acc = __builtin_fmaf(k.y, e, acc);
      const float oe = k.y * e;
      const float tx = __builtin_fmaf(u.w + u.w, dx, q1);
      const float ty = __builtin_fmaf(v.x, dx, __builtin_fmaf(v.z + v.z, dy, v.w * dz));
      const float tz = __builtin_fmaf(v.y, dx, __builtin_fmaf(v.w, dy, (k.x + k.x) * dz));
      sx = __builtin_fmaf(oe, tx, sx);
      sy = __builtin_fmaf(oe, ty, sy);
      sz = __builtin_fmaf(oe, tz, sz);
      cr = __builtin_fmaf(oe, col.x, cr);
      cg = __builtin_fmaf(oe, col.y, cg);
      cb = __builtin_fmaf(oe, col.z, cb);
    }
  }
  if (!live) return;
  if (out.density) out.density[i] = acc;
  if (out.normal) {
    // scaled by the largest component first: the squares of a G that is finite and not zero neither underflow nor overflow
    const float m = fmaxf(fmaxf(fabsf(sx), fabsf(sy)), fabsf(sz));
    const bool ok = m > 0.0f && isfinite(sx) && isfinite(sy) && isfinite(sz);
    const float ux = sx / m, uy = sy / m, uz = sz / m;
    const float inv = -1.0f / sqrtf((ux * ux + uy * uy) + uz * uz);
    out.normal[3 * (size_t)i] = ok ? ux * inv : 0.0f;
    out.normal[3 * (size_t)i + 1] = ok ? uy * inv : 0.0f;
    out.normal[3 * (size_t)i + 2] = ok ? uz * inv : 0.0f;
  }
  if (out.color) {
    const bool any = acc != 0.0f;
    out.color[3 * (size_t)i] = any ? cr / acc : 0.0f;
    out.color[3 * (size_t)i + 1] = any ? cg / acc : 0.0f;
    out.color[3 * (size_t)i + 2] = any ? cb / acc : 0.0f;
  }
}
