// mesh.hip - closest point and signed distance of query points to a triangle mesh: the `cubvh.cuBVH(vertices, faces)
// .signed_distance(points, return_uvw=True, mode="raystab")` the reference calls once per avatar to anchor its Gaussians
// on the body mesh (/root/reference/animation.py:333-378).  cubvh is a CUDA-only extension; this is the HIP stand-in.
//
// Contract (include/hgs_rast.h, hgs_mesh_query):
//   closest face = argmin over the faces of (fp32 squared point-triangle distance, face index) in lexicographic order;
//   faces whose fp32 cross(v1 - v0, v2 - v0) is exactly zero (or not finite, or with an index outside [0, V)) are skipped;
//   uvw = barycentric weights of the closest point (Ericson's region-based closest point on a triangle), dist = sqrt(d2);
//   raystab: the point is inside iff all 64 rays +-d_i (32 fixed Fibonacci-lattice directions) hit a face at t > 0
//   (watertight ray / triangle test), and then dist is negated.
//
// Acceleration, MI355X-first and without a host round trip inside a query (the knn.hip pattern; box, grid fit and scan are
// gridscan.h's):
//   plan   bounding box of the finite vertices (wave max, one ordered-integer atomic per wave and axis), a uniform grid
//          sized on the device from it (cell edge cbrt(vol / 8F): ~1-4 faces per occupied cell of a body mesh), and the
//          number of (face, cell) references when every face is binned into the cells of its bounding box;
//   build  (sized by the host from the plan's header) the triangles packed as 3 float4 each, count / exclusive scan /
//          scatter of the references into per-cell face lists (order inside a cell arbitrary: no result depends on it);
//   query  one thread per point.  Closest point: shells of cells around the point's cell (clamped into the grid for
//          points outside the box) until no unsearched cell can hold anything as close (the knn.hip stop rule with a
//          margin for fp32 rounding) - exact: the brute force's face, uvw and dist, ties included.  Ray stab: a slab walk
//          along the ray's major axis that visits every cell the ray passes within 0.02 cells of, any-hit per ray, the
//          first escaping ray ends an outside point - conservative, so the inside test equals the brute force's.
// The brute force (hgs_k_mesh_query_brute) evaluates the same __device__ functions over all faces: the check and the
// fallback.  No scratch memory (no per-thread stack: the grid needs none), no LDS.
#include "hgs_common.h"

#define HGS_MESH_MAX_CELLS (1u << 22)
#define HGS_MESH_RAY_MARGIN 0.02f        // cells: the slab walk's widening (>> the fp32 error of a cell coordinate)

// first bytes of the grid buffer (written by hgs_k_mesh_grid_init from the host's copy of the plan)
struct MeshGridHdr {
  int32_t gx, gy, gz;
  uint32_t ncells;
  float ox, oy, oz, h, inv_h;
  float cmax;                          // largest |coordinate| of the box corners (rounding margin of the stop rule)
  int32_t F;
  uint32_t nrefs;
  unsigned long long off_tris, off_start, off_cursor, off_bsum, off_refs;   // byte offsets inside the grid buffer
};

__device__ __forceinline__ float3 m3sub(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float m3dot(float3 a, float3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float m3sel(float3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }
__device__ __forceinline__ bool m3finite(float3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// The face as every path sees it.  false: skipped (index outside [0, V), cross product exactly zero or not finite).
__device__ __forceinline__ bool mesh_face(int V, const float* __restrict__ vtx, const int32_t* __restrict__ faces, int f,
                                          float3& a, float3& b, float3& c) {
  const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  a = make_float3(vtx[3 * (size_t)i0], vtx[3 * (size_t)i0 + 1], vtx[3 * (size_t)i0 + 2]);
  b = make_float3(vtx[3 * (size_t)i1], vtx[3 * (size_t)i1 + 1], vtx[3 * (size_t)i1 + 2]);
  c = make_float3(vtx[3 * (size_t)i2], vtx[3 * (size_t)i2 + 1], vtx[3 * (size_t)i2 + 2]);
  const float3 e1 = m3sub(b, a), e2 = m3sub(c, a);
  const float nx = e1.y * e2.z - e1.z * e2.y, ny = e1.z * e2.x - e1.x * e2.z, nz = e1.x * e2.y - e1.y * e2.x;
  if (nx == 0.0f && ny == 0.0f && nz == 0.0f) return false;
  return isfinite(nx) && isfinite(ny) && isfinite(nz);
}

// THE closest point on triangle (a, b, c) to p (Ericson, Real-Time Collision Detection 5.1.5): returns the squared
// distance, v and w (u = 1 - v - w; all three >= 0).  Every query path goes through this function.
__device__ __forceinline__ float mesh_closest_on_tri(float3 p, float3 a, float3 b, float3 c, float& v, float& w) {
  const float3 ab = m3sub(b, a), ac = m3sub(c, a), ap = m3sub(p, a);
  const float d1 = m3dot(ab, ap), d2 = m3dot(ac, ap);
  const float3 bp = m3sub(p, b);
  const float d3 = m3dot(ab, bp), d4 = m3dot(ac, bp);
  const float3 cp = m3sub(p, c);
  const float d5 = m3dot(ab, cp), d6 = m3dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0f && d2 <= 0.0f) { v = 0.0f; w = 0.0f; }                                    // vertex a
  else if (d3 >= 0.0f && d4 <= d3) { v = 1.0f; w = 0.0f; }                                  // vertex b
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { v = d1 / (d1 - d3); w = 0.0f; }        // edge ab
  else if (d6 >= 0.0f && d5 <= d6) { v = 0.0f; w = 1.0f; }                                  // vertex c
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { v = 0.0f; w = d2 / (d2 - d6); }        // edge ac
  else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {                          // edge bc
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    v = 1.0f - w;
  } else {                                                                                  // interior
    const float inv = 1.0f / ((va + vb) + vc);
    v = fmaxf(vb * inv, 0.0f);
    w = fmaxf(vc * inv, 0.0f);
  }
  const float3 q = make_float3((a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w);
  const float3 d = m3sub(p, q);
  return m3dot(d, d);
}

struct MeshBest {
  float d2, v, w;
  int f;
};

__device__ __forceinline__ void mesh_consider(MeshBest& B, float3 p, float3 a, float3 b, float3 c, int f) {
  float v, w;
  const float d2 = mesh_closest_on_tri(p, a, b, c, v, w);
  if (d2 < B.d2 || (d2 == B.d2 && f < B.f)) { B.d2 = d2; B.v = v; B.w = w; B.f = f; }     // (d2, face) lexicographic
}

// Fixed ray directions: z_i = 1 - (2i + 1) / 32, theta_i = 2 pi frac(0.6180339887 i + 0.1234)
__device__ __forceinline__ float3 mesh_ray_dir(int i) {
  const float z = 1.0f - (float)(2 * i + 1) / 32.0f;
  const float r = sqrtf(fmaxf(1.0f - z * z, 0.0f));
  const float fr = 0.6180339887f * (float)i + 0.1234f;
  const float th = 6.283185307179586f * (fr - floorf(fr));
  float s, co;
  sincosf(th, &s, &co);
  return make_float3(r * co, r * s, z);
}

// Watertight ray / triangle intersection (Woop, Benthin, Wald, JCGT 2013): shear into the ray's frame, three edge
// functions, recomputed in fp64 when one is exactly zero - a ray through a shared edge or vertex hits at least one of
// the triangles that share it.  Any hit with t > 0, either winding.
struct MeshRay {
  float3 o;
  int kx, ky, kz;
  float sx, sy, sz;
};

__device__ __forceinline__ MeshRay mesh_ray(float3 o, float3 d) {
  MeshRay r;
  r.o = o;
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
  r.kx = r.kz == 2 ? 0 : r.kz + 1;
  r.ky = r.kx == 2 ? 0 : r.kx + 1;
  const float dz = m3sel(d, r.kz);
  if (dz < 0.0f) { const int t = r.kx; r.kx = r.ky; r.ky = t; }
  r.sx = m3sel(d, r.kx) / dz;
  r.sy = m3sel(d, r.ky) / dz;
  r.sz = 1.0f / dz;
  return r;
}

__device__ __forceinline__ bool mesh_ray_hits(const MeshRay& r, float3 a, float3 b, float3 c) {
  const float3 A = m3sub(a, r.o), B = m3sub(b, r.o), C = m3sub(c, r.o);
  const float Akz = m3sel(A, r.kz), Bkz = m3sel(B, r.kz), Ckz = m3sel(C, r.kz);
  const float Ax = m3sel(A, r.kx) - r.sx * Akz, Ay = m3sel(A, r.ky) - r.sy * Akz;
  const float Bx = m3sel(B, r.kx) - r.sx * Bkz, By = m3sel(B, r.ky) - r.sy * Bkz;
  const float Cx = m3sel(C, r.kx) - r.sx * Ckz, Cy = m3sel(C, r.ky) - r.sy * Ckz;
  float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
  if (U == 0.0f || V == 0.0f || W == 0.0f) {
    U = (float)((double)Cx * (double)By - (double)Cy * (double)Bx);
    V = (float)((double)Ax * (double)Cy - (double)Ay * (double)Cx);
    W = (float)((double)Bx * (double)Ay - (double)By * (double)Ax);
  }
  if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
  const float det = (U + V) + W;
  if (det == 0.0f) return false;
  const float T = (U * (r.sz * Akz) + V * (r.sz * Bkz)) + W * (r.sz * Ckz);
  return det > 0.0f ? T > 0.0f : T < 0.0f;
}

__device__ __forceinline__ void mesh_write(int i, const MeshBest& B, bool inside, float* __restrict__ dist,
                                           int32_t* __restrict__ face, float* __restrict__ uvw) {
  const bool found = B.f != 0x7fffffff;
  const float d = sqrtf(B.d2);
  dist[i] = found ? (inside ? -d : d) : __int_as_float(0x7fc00000);
  face[i] = found ? B.f : -1;
  if (uvw) {
    const float u = found ? fmaxf(1.0f - B.v - B.w, 0.0f) : 0.0f;
    uvw[3 * (size_t)i] = u;
    uvw[3 * (size_t)i + 1] = found ? B.v : 0.0f;
    uvw[3 * (size_t)i + 2] = found ? B.w : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ plan

extern "C" __global__ void __launch_bounds__(256)
hgs_k_mesh_bbox(int V, const float* __restrict__ vtx, hgs_mesh_grid_info* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float3 p = make_float3(0.f, 0.f, 0.f);
  if (i < V) p = make_float3(vtx[3 * (size_t)i], vtx[3 * (size_t)i + 1], vtx[3 * (size_t)i + 2]);
  hgs_box_reduce(i < V && m3finite(p), p.x, p.y, p.z, info->bmin, info->bmax);     // non-finite vertices do not stretch the box
}

// one thread: the grid from the box (gridscan.h), first cell edge cbrt(vol / 8F), at most min(16 F, 4 M) cells
extern "C" __global__ void hgs_k_mesh_grid_setup(int F, hgs_mesh_grid_info* __restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool empty = info->bmin[0] > info->bmax[0];     // no finite vertex
  float lo[3], ext[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = empty ? 0.0f : hgs_key_float(info->bmin[a]);
    ext[a] = empty ? 0.0f : hgs_key_float(info->bmax[a]) - lo[a];
    if (!(ext[a] >= 0.0f) || !(ext[a] < 3.0e38f)) ext[a] = 0.0f;
  }
  const uint32_t nc_max = (uint32_t)min(max(16ll * F, 64ll), (long long)HGS_MESH_MAX_CELLS);
  const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
  float h = 1.0f;
  uint32_t g[3] = {1u, 1u, 1u};
  if (emax > 0.0f) {
    h = hgs_grid_fit(ext, cbrtf(hgs_grid_volume(ext, emax) / (8.0f * (float)F)), nc_max, g);
    if ((unsigned long long)g[0] * g[1] * g[2] > nc_max) { g[0] = g[1] = g[2] = 1u; h = emax; }   // (cannot happen)
  }
  for (int a = 0; a < 3; ++a) { info->dims[a] = (int32_t)g[a]; info->origin[a] = lo[a]; }
  info->ncells = g[0] * g[1] * g[2];
  info->cell = h;
  info->num_faces = F;
  info->reserved0 = 0;
}

struct MeshCells { int x0, y0, z0, x1, y1, z1; };

// cells of the face's bounding box (the same fp32 operations at plan, build and query time)
__device__ __forceinline__ MeshCells mesh_face_cells(float3 a, float3 b, float3 c, const float o[3], float inv_h,
                                                     const int g[3]) {
  MeshCells r;
  r.x0 = hgs_grid_cell1(fminf(a.x, fminf(b.x, c.x)), o[0], inv_h, g[0]);
  r.x1 = hgs_grid_cell1(fmaxf(a.x, fmaxf(b.x, c.x)), o[0], inv_h, g[0]);
  r.y0 = hgs_grid_cell1(fminf(a.y, fminf(b.y, c.y)), o[1], inv_h, g[1]);
  r.y1 = hgs_grid_cell1(fmaxf(a.y, fmaxf(b.y, c.y)), o[1], inv_h, g[1]);
  r.z0 = hgs_grid_cell1(fminf(a.z, fminf(b.z, c.z)), o[2], inv_h, g[2]);
  r.z1 = hgs_grid_cell1(fmaxf(a.z, fmaxf(b.z, c.z)), o[2], inv_h, g[2]);
  return r;
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_mesh_count_refs(int V, const float* __restrict__ vtx, int F, const int32_t* __restrict__ faces,
                      hgs_mesh_grid_info* __restrict__ info) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  const float o[3] = {info->origin[0], info->origin[1], info->origin[2]};
  const int g[3] = {info->dims[0], info->dims[1], info->dims[2]};
  const float inv_h = 1.0f / info->cell;
  unsigned long long n = 0;
  float3 a, b, c;
  if (f < F && mesh_face(V, vtx, faces, f, a, b, c)) {
    const MeshCells r = mesh_face_cells(a, b, c, o, inv_h, g);
    n = (unsigned long long)(r.x1 - r.x0 + 1) * (unsigned long long)(r.y1 - r.y0 + 1) * (unsigned long long)(r.z1 - r.z0 + 1);
  }
  for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd((unsigned long long*)&info->num_refs, n);
}

// ------------------------------------------------------------------------------------------------ build

struct MeshGridPtrs {
  float4* tris;
  uint32_t* start;
  uint32_t* cursor;
  uint32_t* bsum;
  uint32_t* refs;
};

__device__ __forceinline__ MeshGridPtrs mesh_ptrs(const MeshGridHdr& G, void* grid) {
  char* gp = static_cast<char*>(grid);
  return {reinterpret_cast<float4*>(gp + G.off_tris), reinterpret_cast<uint32_t*>(gp + G.off_start),
          reinterpret_cast<uint32_t*>(gp + G.off_cursor), reinterpret_cast<uint32_t*>(gp + G.off_bsum),
          reinterpret_cast<uint32_t*>(gp + G.off_refs)};
}

// header, zeroed cell counts, packed triangles (v0.w = face index, or -1 when the face is skipped)
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mesh_grid_init(MeshGridHdr G, int V, const float* __restrict__ vtx, const int32_t* __restrict__ faces, void* grid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const MeshGridPtrs p = mesh_ptrs(G, grid);
  if (i == 0) *static_cast<MeshGridHdr*>(grid) = G;
  if (i <= (long long)G.ncells) p.start[i] = 0u;
  if (i < G.F) {
    float3 a = make_float3(0.f, 0.f, 0.f), b = a, c = a;
    const bool ok = mesh_face(V, vtx, faces, (int)i, a, b, c);
    p.tris[3 * i] = make_float4(a.x, a.y, a.z, __int_as_float(ok ? (int)i : -1));
    p.tris[3 * i + 1] = make_float4(b.x, b.y, b.z, 0.f);
    p.tris[3 * i + 2] = make_float4(c.x, c.y, c.z, 0.f);
  }
}

__device__ __forceinline__ bool mesh_tri(const float4* __restrict__ tris, int f, float3& a, float3& b, float3& c) {
  const float4 t0 = tris[3 * (size_t)f], t1 = tris[3 * (size_t)f + 1], t2 = tris[3 * (size_t)f + 2];
  a = make_float3(t0.x, t0.y, t0.z); b = make_float3(t1.x, t1.y, t1.z); c = make_float3(t2.x, t2.y, t2.z);
  return __float_as_int(t0.w) >= 0;
}

// pass 0: count the references of every cell; pass 1: scatter the face indices into the cells' lists
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mesh_bin(MeshGridHdr G, void* grid, int pass) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= G.F) return;
  const MeshGridPtrs p = mesh_ptrs(G, grid);
  float3 a, b, c;
  if (!mesh_tri(p.tris, f, a, b, c)) return;
  const float o[3] = {G.ox, G.oy, G.oz};
  const int g[3] = {G.gx, G.gy, G.gz};
  const MeshCells r = mesh_face_cells(a, b, c, o, G.inv_h, g);
  for (int z = r.z0; z <= r.z1; ++z)
    for (int y = r.y0; y <= r.y1; ++y)
      for (int x = r.x0; x <= r.x1; ++x) {
        const uint32_t cell = ((uint32_t)z * (uint32_t)G.gy + (uint32_t)y) * (uint32_t)G.gx + (uint32_t)x;
        if (pass == 0) {
          atomicAdd(&p.start[cell], 1u);
        } else {
          const uint32_t slot = atomicAdd(&p.cursor[cell], 1u);
          if (slot < G.nrefs) p.refs[slot] = (uint32_t)f;        // (bounded even if the vertices changed since the plan)
        }
      }
}

// exclusive scan of start[0 .. ncells) in place (start[ncells] = total): the three passes of gridscan.h
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mesh_scan1(MeshGridHdr G, void* grid) {
  const MeshGridPtrs p = mesh_ptrs(G, grid);
  hgs_scan_totals(G.ncells, p.start, p.bsum);
}
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mesh_scan2(MeshGridHdr G, void* grid) {
  const MeshGridPtrs p = mesh_ptrs(G, grid);
  hgs_scan_carry((G.ncells + HGS_SCAN_BLOCK - 1u) / HGS_SCAN_BLOCK, p.bsum, p.bsum);
}
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mesh_scan3(MeshGridHdr G, void* grid) {
  const MeshGridPtrs p = mesh_ptrs(G, grid);
  const uint32_t n = G.ncells;
  uint32_t i, ex, v;
  if (hgs_scan_prefix(n, p.start, p.bsum, i, ex, v)) { p.start[i] = ex; p.cursor[i] = ex; }
  if (i == n - 1u) p.start[n] = ex + v;
}

// ------------------------------------------------------------------------------------------------ query

// every (valid) face listed in cell c
template <class Fn>
__device__ __forceinline__ bool mesh_cell_faces(const MeshGridHdr& G, const MeshGridPtrs& p, uint32_t c, Fn&& fn) {
  const uint32_t s = p.start[c], e = min(p.start[c + 1u], G.nrefs);
  for (uint32_t k = s; k < e; ++k) {
    const uint32_t f = p.refs[k];
    if (f >= (uint32_t)G.F) continue;
    float3 a, b, c3;
    if (!mesh_tri(p.tris, (int)f, a, b, c3)) continue;
    if (fn(a, b, c3, (int)f)) return true;
  }
  return false;
}

// Closest face through the grid: shells of cells at Chebyshev distance r around the point's (clamped) cell.  A face
// not yet seen lies entirely outside the block [c - r, c + r]^3 of cells, so at least `reach` away; the search stops
// once the best squared distance is below reach^2.  reach is shortened by 1e-3 cells (a cell index is floor((x - o) /
// h) in fp32) and by 1e-5 of the largest coordinate in play (the fp32 error of a computed point-triangle distance),
// so a face beyond the block never ties or beats the best - the result equals the brute force's, ties included.
__device__ __forceinline__ MeshBest mesh_grid_closest(const MeshGridHdr& G, const MeshGridPtrs& p, float3 q) {
  MeshBest B = {__int_as_float(0x7f800000), 0.0f, 0.0f, 0x7fffffff};
  const int gx = G.gx, gy = G.gy, gz = G.gz;
  const int cx = hgs_grid_cell1(q.x, G.ox, G.inv_h, gx), cy = hgs_grid_cell1(q.y, G.oy, G.inv_h, gy),
            cz = hgs_grid_cell1(q.z, G.oz, G.inv_h, gz);
  const float rx = q.x - G.ox, ry = q.y - G.oy, rz = q.z - G.oz;
  const float margin = 1e-3f * G.h + 1e-5f * fmaxf(G.cmax, fmaxf(fabsf(q.x), fmaxf(fabsf(q.y), fabsf(q.z))));
  auto consider = [&](float3 a, float3 b, float3 c, int f) { mesh_consider(B, q, a, b, c, f); return false; };
  const int rmax = max(gx, max(gy, gz));
  for (int r = 0; r <= rmax; ++r) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, gz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, gy - 1);
    const int x0 = max(cx - r, 0), x1 = min(cx + r, gx - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const uint32_t row = ((uint32_t)z * (uint32_t)gy + (uint32_t)y) * (uint32_t)gx;
        if (abs(z - cz) == r || abs(y - cy) == r) {
          for (int x = x0; x <= x1; ++x) mesh_cell_faces(G, p, row + (uint32_t)x, consider);
        } else {
          if (cx - r >= 0) mesh_cell_faces(G, p, row + (uint32_t)(cx - r), consider);
          if (r > 0 && cx + r <= gx - 1) mesh_cell_faces(G, p, row + (uint32_t)(cx + r), consider);
        }
      }
    if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == gx - 1 && y1 == gy - 1 && z1 == gz - 1) break;      // the whole grid
    float reach = __int_as_float(0x7f800000);
    if (cx - r > 0) reach = fminf(reach, rx - (float)(cx - r) * G.h);
    if (cx + r < gx - 1) reach = fminf(reach, (float)(cx + r + 1) * G.h - rx);
    if (cy - r > 0) reach = fminf(reach, ry - (float)(cy - r) * G.h);
    if (cy + r < gy - 1) reach = fminf(reach, (float)(cy + r + 1) * G.h - ry);
    if (cz - r > 0) reach = fminf(reach, rz - (float)(cz - r) * G.h);
    if (cz + r < gz - 1) reach = fminf(reach, (float)(cz + r + 1) * G.h - rz);
    reach -= margin;
    if (reach > 0.0f && B.d2 < reach * reach) break;
  }
  return B;
}

// Any hit of the ray q + t d (t > 0) through the grid.  A slab walk along the ray's major axis k in cell units: for
// every slab of cells [j, j + 1) of axis k the ray crosses, the cells of the two other axes that the ray segment
// inside the slab touches, everything widened by HGS_MESH_RAY_MARGIN cells.  A face the ray hits contains the hit
// point, so the hit point's cell is one of the face's cells (up to fp32 rounding far below the margin): the walk tests
// every face the brute force would find a hit with (and maybe a few more, which changes nothing for any-hit).
__device__ bool mesh_grid_ray_hits(const MeshGridHdr& G, const MeshGridPtrs& p, float3 q, float3 d) {
  const MeshRay ray = mesh_ray(q, d);
  auto hit = [&](float3 a, float3 b, float3 c, int) { return mesh_ray_hits(ray, a, b, c); };
  const float m = HGS_MESH_RAY_MARGIN;
  const float u[3] = {(q.x - G.ox) * G.inv_h, (q.y - G.oy) * G.inv_h, (q.z - G.oz) * G.inv_h};
  const float dd[3] = {d.x, d.y, d.z};
  const int g[3] = {G.gx, G.gy, G.gz};
  // the ray's parameter range inside the (widened) grid box
  float s0 = 0.0f, s1 = __int_as_float(0x7f800000);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (dd[a] != 0.0f) {
      const float t1 = (-m - u[a]) / dd[a], t2 = ((float)g[a] + m - u[a]) / dd[a];
      s0 = fmaxf(s0, fminf(t1, t2));
      s1 = fminf(s1, fmaxf(t1, t2));
    } else if (!(u[a] >= -m && u[a] <= (float)g[a] + m)) {
      return false;
    }
  }
  if (!(s0 <= s1)) return false;
  const int k = ray.kz, ka = k == 0 ? 1 : 0, kb = k == 2 ? 1 : 2;
  const float uk = k == 0 ? u[0] : (k == 1 ? u[1] : u[2]), dk = k == 0 ? dd[0] : (k == 1 ? dd[1] : dd[2]);
  const float ua = ka == 0 ? u[0] : u[1], da = ka == 0 ? dd[0] : dd[1];
  const float ub = kb == 1 ? u[1] : u[2], db = kb == 1 ? dd[1] : dd[2];
  const int gk = k == 0 ? g[0] : (k == 1 ? g[1] : g[2]), ga = ka == 0 ? g[0] : g[1], gb = kb == 1 ? g[1] : g[2];
  const float xk0 = uk + s0 * dk, xk1 = uk + s1 * dk;
  const int step = dk > 0.0f ? 1 : -1;
  int j = (int)floorf(dk > 0.0f ? xk0 - m : xk0 + m), jend = (int)floorf(dk > 0.0f ? xk1 + m : xk1 - m);
  j = min(max(j, 0), gk - 1);
  jend = min(max(jend, 0), gk - 1);
  const float inv_dk = 1.0f / dk;
  for (;; j += step) {
    // the ray's parameters inside slab j (widened), clipped to [s0, s1]
    const float ta = ((float)j - m - uk) * inv_dk, tb = ((float)(j + 1) + m - uk) * inv_dk;
    const float sa = fmaxf(fminf(ta, tb), s0), sb = fminf(fmaxf(ta, tb), s1);
    if (sa <= sb) {
      const float pa0 = ua + sa * da, pa1 = ua + sb * da, pb0 = ub + sa * db, pb1 = ub + sb * db;
      const int a0 = min(max((int)floorf(fminf(pa0, pa1) - m), 0), ga - 1), a1 = min(max((int)floorf(fmaxf(pa0, pa1) + m), 0), ga - 1);
      const int b0 = min(max((int)floorf(fminf(pb0, pb1) - m), 0), gb - 1), b1 = min(max((int)floorf(fmaxf(pb0, pb1) + m), 0), gb - 1);
      for (int ib = b0; ib <= b1; ++ib)
        for (int ia = a0; ia <= a1; ++ia) {
          const int x = k == 0 ? j : ia, y = k == 1 ? j : (ka == 1 ? ia : ib), z = k == 2 ? j : ib;
          const uint32_t cell = ((uint32_t)z * (uint32_t)G.gy + (uint32_t)y) * (uint32_t)G.gx + (uint32_t)x;
          if (mesh_cell_faces(G, p, cell, hit)) return true;
        }
    }
    if (j == jend) break;
  }
  return false;
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_mesh_query_grid(int P, const float* __restrict__ pts, const void* __restrict__ grid, int mode,
                      float* __restrict__ dist, int32_t* __restrict__ face, float* __restrict__ uvw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const MeshGridHdr G = *static_cast<const MeshGridHdr*>(grid);
  const MeshGridPtrs p = mesh_ptrs(G, const_cast<void*>(grid));
  const float3 q = make_float3(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
  MeshBest B = {0.0f, 0.0f, 0.0f, 0x7fffffff};
  bool inside = false;
  if (m3finite(q)) {
    B = mesh_grid_closest(G, p, q);
    if (mode == HGS_MESH_RAYSTAB && B.f != 0x7fffffff) {
      inside = true;
      for (int r = 0; r < 64 && inside; ++r) {
        const float3 d = mesh_ray_dir(r >> 1);
        inside = mesh_grid_ray_hits(G, p, q, (r & 1) ? make_float3(-d.x, -d.y, -d.z) : d);
      }
    }
  }
  mesh_write(i, B, inside, dist, face, uvw);
}

// The brute force: every face for every point, the same __device__ functions in the same order of decisions.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_mesh_query_brute(int P, const float* __restrict__ pts, int V, const float* __restrict__ vtx, int F,
                       const int32_t* __restrict__ faces, int mode, float* __restrict__ dist, int32_t* __restrict__ face,
                       float* __restrict__ uvw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float3 q = make_float3(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
  MeshBest B = {__int_as_float(0x7f800000), 0.0f, 0.0f, 0x7fffffff};
  bool inside = false;
  if (m3finite(q)) {
    for (int f = 0; f < F; ++f) {
      float3 a, b, c;
      if (mesh_face(V, vtx, faces, f, a, b, c)) mesh_consider(B, q, a, b, c, f);
    }
    if (mode == HGS_MESH_RAYSTAB && B.f != 0x7fffffff) {
      inside = true;
      for (int r = 0; r < 64 && inside; ++r) {
        const float3 d = mesh_ray_dir(r >> 1);
        const MeshRay ray = mesh_ray(q, (r & 1) ? make_float3(-d.x, -d.y, -d.z) : d);
        bool hit = false;
        for (int f = 0; f < F && !hit; ++f) {
          float3 a, b, c;
          hit = mesh_face(V, vtx, faces, f, a, b, c) && mesh_ray_hits(ray, a, b, c);
        }
        inside = hit;
      }
    }
  }
  mesh_write(i, B, inside, dist, face, uvw);
}
