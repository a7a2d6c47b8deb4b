// meshview.hip - the mesh view: a forward triangle rasterizer for the body mesh (include/hgs_rast.h: hgs_meshview_* states
// the vertex stage, the exact integer coverage rule, the fragment arithmetic and the vertex normals).
//
// Reference code replaced: render_mesh_normal of the reference's animation.py:558-601 (nvdiffrast's rasterize and
// interpolate around three scatter_add_ calls), forward only.
//
//   hgs_k_mv_normals      a thread per (mesh, vertex): the face normals of its CSR adjacency summed in order (a gather)
//   hgs_k_mv_vertex       a thread per (view, vertex): the 16-byte record {x_fix, y_fix, bits(zw), bits(invw)}
//   hgs_k_mv_count        a thread per (view, face): the box of 16 x 16 pixel tiles its samples can lie in, one count per
//                         tile of the box, the call's total in 64 bits
//   hgs_k_mv_scan1..3     the device-wide exclusive scan of gridscan.h over the B * tiles counts
//   hgs_k_mv_fill         a thread per (view, face): claims a slot in every tile of its box (integer atomics; the order of
//                         a list is arbitrary and the draw does not depend on it)
//   hgs_k_mv_draw         grid (tiles, B), 256 threads = the tile's pixels.  The list is staged through LDS in batches of
//                         HGS_MESHVIEW_LIST_BATCH: thread t sets up triangle t of the batch ONCE for the tile - the edge
//                         functions at the tile's first sample and their per-unit steps, the ownership bits, 1 / A, the
//                         tile's rows and columns inside the box of its corners.  A wave (four rows of the tile) culls 64
//                         triangles at a time against its rows, one per lane, and walks the survivors of the ballot; a
//                         pixel evaluates an edge function as E(tile origin) + dx step_x + dy step_y, two 32 x 32 -> 64
//                         bit multiply-adds, exact.  int64 -> fp32 conversions, the depth and the winner test run only for
//                         covered samples; u and v are divided out once per pixel, for the winner.  A tile with an empty
//                         list (about 90 % of them for a body at 800 x 800) only writes its background.
//   hgs_k_mv_interpolate  a thread per pixel of a stored rast
// No workgroup waits on another one.  16 x 16 tiles: a body triangle at 800 x 800 covers a few pixels, so a larger tile
// only lengthens the lists every pixel walks; 256 threads with 20 KB of LDS leave several workgroups per CU.  The
// shape is a judgement, not a measured optimum.
#include "hgs_common.h"
#include "gridscan.h"

#define HGS_MV_THREADS 256
#define HGS_MV_INVALID ((int)0x80000000)
#define HGS_MV_NOBOX 0x000000ffu       // tx0 = 255 > tx1 = 0: no tile
#define HGS_MV_COORD_MAX 8388608.0f    // 2^23
#define HGS_MV_TILE_UNITS (HGS_MESHVIEW_TILE * 256)

struct MvPlanPtrs {
  uint32_t* tribox;   // [B][F]: tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24, or HGS_MV_NOBOX
  uint32_t* start;    // [B * tiles + 1]: counts, then their exclusive scan
  uint32_t* cursor;   // [B * tiles]
  uint32_t* bsum;
};

__device__ __forceinline__ float mv_safe_normalise(float& x, float& y, float& z) {
  const float dot = (x * x + y * y) + z * z;
  if (!(dot > 1e-20f)) { x = 0.0f; y = 0.0f; z = 1.0f; return dot; }
  const float len = sqrtf(fmaxf(dot, 1e-20f));      // (correctly rounded; __fsqrt_rn is the approximate v_sqrt_f32 here)
  x = __fdiv_rn(x, len); y = __fdiv_rn(y, len); z = __fdiv_rn(z, len);
  return dot;
}

extern "C" __global__ void __launch_bounds__(HGS_MV_THREADS)
hgs_k_mv_normals(const hgs_meshview_args a, int Bv) {
  const long long i = (long long)blockIdx.x * HGS_MV_THREADS + threadIdx.x;
  if (i >= (long long)Bv * a.V) return;
  const int b = (int)(i / a.V), v = (int)(i - (long long)b * a.V);
  const float* __restrict__ vtx = a.vertices + (size_t)b * (size_t)a.vertex_stride;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  const int s = a.adj_start[v], e = a.adj_start[v + 1];
  for (int k = s; k < e; ++k) {
    const int f = a.adj[k] / 3;
    if ((unsigned)f >= (unsigned)a.F) continue;
    const int i0 = a.faces[3 * (size_t)f], i1 = a.faces[3 * (size_t)f + 1], i2 = a.faces[3 * (size_t)f + 2];
    if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) continue;
    const float* p0 = vtx + 3 * (size_t)i0;
    const float* p1 = vtx + 3 * (size_t)i1;
    const float* p2 = vtx + 3 * (size_t)i2;
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    nx = nx + (e1y * e2z - e1z * e2y);
    ny = ny + (e1z * e2x - e1x * e2z);
    nz = nz + (e1x * e2y - e1y * e2x);
  }
  mv_safe_normalise(nx, ny, nz);
  float* o = a.normals + 3 * (size_t)i;
  o[0] = nx; o[1] = ny; o[2] = nz;
}

extern "C" __global__ void __launch_bounds__(HGS_MV_THREADS)
hgs_k_mv_vertex(const hgs_meshview_args a) {
  const long long i = (long long)blockIdx.x * HGS_MV_THREADS + threadIdx.x;
  if (i >= (long long)a.B * a.V) return;
  const int b = (int)(i / a.V), v = (int)(i - (long long)b * a.V);
  const float* __restrict__ m = a.mvp + (size_t)b * 16;
  const float* __restrict__ p = a.vertices + (size_t)b * (size_t)a.vertex_stride + 3 * (size_t)v;
  const float x = p[0], y = p[1], z = p[2];
  float c[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
  const float invw = __fdiv_rn(1.0f, c[3]);
  const float xs = ((c[0] * invw) * 0.5f + 0.5f) * (float)(a.W << 8);
  const float ys = ((c[1] * invw) * 0.5f + 0.5f) * (float)(a.H << 8);
  const float zw = c[2] * invw;
  // (a NaN fails every comparison, an infinity the bound)
  const bool ok = c[3] > 0.0f && fabsf(xs) < HGS_MV_COORD_MAX && fabsf(ys) < HGS_MV_COORD_MAX && fabsf(zw) <= 3.402823466e38f;
  int4 r = make_int4(HGS_MV_INVALID, 0, 0, 0);
  if (ok) r = make_int4((int)rintf(xs), (int)rintf(ys), __float_as_int(zw), __float_as_int(invw));
  reinterpret_cast<int4*>(a.records)[i] = r;
}

// the three records of face f of a view; false: an index outside [0, V) or an invalid vertex
__device__ __forceinline__ bool mv_tri_load(const int4* __restrict__ rec, const int32_t* __restrict__ faces, int V, int f,
                                            int4& ra, int4& rb, int4& rc) {
  const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  ra = rec[i0]; rb = rec[i1]; rc = rec[i2];
  return ra.x != HGS_MV_INVALID && rb.x != HGS_MV_INVALID && rc.x != HGS_MV_INVALID;
}

__device__ __forceinline__ long long mv_cross(int ux, int uy, int vx, int vy) {
  return (long long)ux * vy - (long long)uy * vx;
}

// tiles whose samples (c 256 + 128, r 256 + 128) can lie inside the triangle's box, clipped to the image
__device__ __forceinline__ uint32_t mv_tri_box(const int4& ra, const int4& rb, const int4& rc, int H, int W) {
  if (mv_cross(rb.x - ra.x, rb.y - ra.y, rc.x - ra.x, rc.y - ra.y) == 0) return HGS_MV_NOBOX;
  const int minx = min(ra.x, min(rb.x, rc.x)), maxx = max(ra.x, max(rb.x, rc.x));
  const int miny = min(ra.y, min(rb.y, rc.y)), maxy = max(ra.y, max(rb.y, rc.y));
  // minx <= c 256 + 128 <= maxx  (arithmetic shifts: floor)
  const int c0 = max((minx + 127) >> 8, 0), c1 = min((maxx - 128) >> 8, W - 1);
  const int r0 = max((miny + 127) >> 8, 0), r1 = min((maxy - 128) >> 8, H - 1);
  if (c0 > c1 || r0 > r1) return HGS_MV_NOBOX;
  return (uint32_t)(c0 / HGS_MESHVIEW_TILE) | ((uint32_t)(c1 / HGS_MESHVIEW_TILE) << 8) |
         ((uint32_t)(r0 / HGS_MESHVIEW_TILE) << 16) | ((uint32_t)(r1 / HGS_MESHVIEW_TILE) << 24);
}

extern "C" __global__ void __launch_bounds__(HGS_MV_THREADS)
hgs_k_mv_count(const hgs_meshview_args a, MvPlanPtrs pp, int tiles_x, uint32_t ntiles) {
  const long long i = (long long)blockIdx.x * HGS_MV_THREADS + threadIdx.x;
  if (i >= (long long)a.B * a.F) return;
  const int b = (int)(i / a.F), f = (int)(i - (long long)b * a.F);
  const int4* rec = reinterpret_cast<const int4*>(a.records) + (size_t)b * a.V;
  int4 ra, rb, rc;
  uint32_t box = HGS_MV_NOBOX;
  if (mv_tri_load(rec, a.faces, a.V, f, ra, rb, rc)) box = mv_tri_box(ra, rb, rc, a.H, a.W);
  pp.tribox[i] = box;
  const int tx0 = box & 255, tx1 = (box >> 8) & 255, ty0 = (box >> 16) & 255, ty1 = box >> 24;
  if (tx0 > tx1) return;
  uint32_t* cnt = pp.start + (size_t)b * ntiles;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&cnt[ty * tiles_x + tx], 1u);
  atomicAdd(reinterpret_cast<unsigned long long*>(&a.info->num_refs),
            (unsigned long long)((tx1 - tx0 + 1) * (ty1 - ty0 + 1)));
}

// exclusive scan of start[0 .. n) in place (start[n] = total): the three passes of gridscan.h
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mv_scan1(MvPlanPtrs pp, uint32_t n) { hgs_scan_totals(n, pp.start, pp.bsum); }
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mv_scan2(MvPlanPtrs pp, uint32_t n) { hgs_scan_carry((n + HGS_SCAN_BLOCK - 1u) / HGS_SCAN_BLOCK, pp.bsum, pp.bsum); }
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_mv_scan3(const hgs_meshview_args a, MvPlanPtrs pp, uint32_t n) {
  uint32_t i, ex, v;
  if (hgs_scan_prefix(n, pp.start, pp.bsum, i, ex, v)) { pp.start[i] = ex; pp.cursor[i] = ex; }
  if (i == n - 1u) pp.start[n] = ex + v;
  if (i == 0u) { a.info->B = a.B; a.info->V = a.V; a.info->F = a.F; a.info->H = a.H; a.info->W = a.W; }
}

extern "C" __global__ void __launch_bounds__(HGS_MV_THREADS)
hgs_k_mv_fill(const hgs_meshview_args a, MvPlanPtrs pp, int tiles_x, uint32_t ntiles, uint32_t nrefs) {
  const long long i = (long long)blockIdx.x * HGS_MV_THREADS + threadIdx.x;
  if (i >= (long long)a.B * a.F) return;
  const int b = (int)(i / a.F), f = (int)(i - (long long)b * a.F);
  const uint32_t box = pp.tribox[i];
  const int tx0 = box & 255, tx1 = (box >> 8) & 255, ty0 = (box >> 16) & 255, ty1 = box >> 24;
  if (tx0 > tx1) return;
  uint32_t* refs = static_cast<uint32_t*>(a.lists);
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) {
      const size_t t = (size_t)b * ntiles + (size_t)(ty * tiles_x + tx);
      const uint32_t slot = atomicAdd(&pp.cursor[t], 1u);
      if (slot < pp.start[t + 1] && slot < nrefs) refs[slot] = (uint32_t)f;      // (bounded whatever the buffers hold)
    }
}

// the value of C channels at (u, v) of face `face` of view b - or the background / zeros where face < 0
__device__ __forceinline__ void mv_shade(const hgs_meshview_args& a, int b, int face, float u, float v, float fill,
                                         bool shade_normals, float* __restrict__ out) {
  const int C = a.C;
  int i0 = -1, i1 = -1, i2 = -1;
  if (face >= 0) { i0 = a.faces[3 * (size_t)face]; i1 = a.faces[3 * (size_t)face + 1]; i2 = a.faces[3 * (size_t)face + 2]; }
  if ((unsigned)i0 >= (unsigned)a.V || (unsigned)i1 >= (unsigned)a.V || (unsigned)i2 >= (unsigned)a.V) {
    for (int c = 0; c < C; ++c) out[c] = fill;
    return;
  }
  const float* __restrict__ at = a.attr + (size_t)b * (size_t)a.attr_stride;
  const float w = (1.0f - u) - v;
  float val[HGS_MESHVIEW_MAX_ATTR];
#pragma unroll
  for (int c = 0; c < HGS_MESHVIEW_MAX_ATTR; ++c)
    val[c] = c < C ? ((u * at[(size_t)i0 * C + c]) + (v * at[(size_t)i1 * C + c])) + (w * at[(size_t)i2 * C + c]) : 0.0f;
  if (shade_normals) {
    mv_safe_normalise(val[0], val[1], val[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) val[c] = (val[c] + 1.0f) * 0.5f;
  }
#pragma unroll
  for (int c = 0; c < HGS_MESHVIEW_MAX_ATTR; ++c)
    if (c < C) out[c] = val[c];
}

// a triangle of a tile's list as the tile's pixels read it: 80 bytes, five 16-byte LDS reads at one address for the wave
struct __attribute__((aligned(16))) MvTri {
  long long E0, E1;       // edge functions 0 and 1 at the tile's first sample
  long long A;            // |area2|
  int bias;               // bit i: edge i does NOT own its boundary
  uint32_t mask;          // the tile's columns (bits 0-15) and rows (16-31) with a sample in the box of the corners
  int st[4];              // dE0/dx, dE0/dy, dE1/dx, dE1/dy per fixed-point unit
  float zw[3], ia;        // depth at the corners, 1 / A
  float iw[3];            // 1 / w at the corners
  int id;
};

extern "C" __global__ void __launch_bounds__(HGS_MV_THREADS)
hgs_k_mv_draw(const hgs_meshview_args a, MvPlanPtrs pp, int tiles_x, uint32_t ntiles, uint32_t nrefs) {
  __shared__ MvTri sTri[HGS_MESHVIEW_LIST_BATCH];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
  const int lx = tid & (HGS_MESHVIEW_TILE - 1), ly = tid / HGS_MESHVIEW_TILE;
  const int px = tx * HGS_MESHVIEW_TILE + lx, py = ty * HGS_MESHVIEW_TILE + ly;
  const bool live = px < a.W && py < a.H;
  const size_t t = (size_t)b * ntiles + blockIdx.x;
  const uint32_t s = min(pp.start[t], nrefs), e = min(pp.start[t + 1], nrefs);
  const uint32_t n = e > s ? e - s : 0u;
  const int4* rec = reinterpret_cast<const int4*>(a.records) + (size_t)b * a.V;
  const uint32_t* refs = static_cast<const uint32_t*>(a.lists);
  const int ox = tx * HGS_MV_TILE_UNITS + 128, oy = ty * HGS_MV_TILE_UNITS + 128;   // the tile's first sample
  const int dx = lx * 256, dy = ly * 256;
  const uint32_t lane_mask = (1u << lx) | (1u << (16 + ly));
  const int lane = tid & 63;
  const uint32_t wave_rows = 0xfu << (16 + 4 * (tid >> 6));       // a wave is four rows of the tile

  float bz = __int_as_float(0x7f800000), bp0 = 0.0f, bp1 = 0.0f, bp2 = 0.0f;
  int bid = 0x7fffffff;
  for (uint32_t k0 = 0; k0 < n; k0 += HGS_MESHVIEW_LIST_BATCH) {
    const int m = (int)min(n - k0, (uint32_t)HGS_MESHVIEW_LIST_BATCH);
    if (k0) __syncthreads();                     // the batch before has been read
    if (tid < m) {
      const uint32_t f = refs[s + k0 + tid];
      int4 ra, rb, rc;
      MvTri T;
      T.E0 = -1; T.E1 = -1; T.A = 0; T.bias = 7; T.mask = 0u; T.ia = 0.0f; T.id = (int)f;
      T.st[0] = T.st[1] = T.st[2] = T.st[3] = 0;
      T.zw[0] = T.zw[1] = T.zw[2] = 0.0f;
      T.iw[0] = T.iw[1] = T.iw[2] = 0.0f;
      if (f < (uint32_t)a.F && mv_tri_load(rec, a.faces, a.V, (int)f, ra, rb, rc)) {
        const long long area2 = mv_cross(rb.x - ra.x, rb.y - ra.y, rc.x - ra.x, rc.y - ra.y);
        if (area2 != 0) {
          const int sg = area2 > 0 ? 1 : -1;
          T.A = area2 > 0 ? area2 : -area2;
          const int d0x = sg * (rc.x - rb.x), d0y = sg * (rc.y - rb.y);
          const int d1x = sg * (ra.x - rc.x), d1y = sg * (ra.y - rc.y);
          const int d2x = sg * (rb.x - ra.x), d2y = sg * (rb.y - ra.y);
          T.E0 = mv_cross(d0x, d0y, ox - rb.x, oy - rb.y);
          T.E1 = mv_cross(d1x, d1y, ox - rc.x, oy - rc.y);
          T.st[0] = -d0y; T.st[1] = d0x; T.st[2] = -d1y; T.st[3] = d1x;
          const bool own0 = d0y > 0 || (d0y == 0 && d0x > 0);
          const bool own1 = d1y > 0 || (d1y == 0 && d1x > 0);
          const bool own2 = d2y > 0 || (d2y == 0 && d2x > 0);
          T.bias = (own0 ? 0 : 1) | (own1 ? 0 : 2) | (own2 ? 0 : 4);
          T.ia = __fdiv_rn(1.0f, (float)T.A);
          // the samples of this tile inside the box of the corners (a sample outside it is outside the triangle)
          const int c0 = max((min(ra.x, min(rb.x, rc.x)) + 127) >> 8, tx * HGS_MESHVIEW_TILE) - tx * HGS_MESHVIEW_TILE;
          const int c1 = min((max(ra.x, max(rb.x, rc.x)) - 128) >> 8, tx * HGS_MESHVIEW_TILE + HGS_MESHVIEW_TILE - 1) - tx * HGS_MESHVIEW_TILE;
          const int r0 = max((min(ra.y, min(rb.y, rc.y)) + 127) >> 8, ty * HGS_MESHVIEW_TILE) - ty * HGS_MESHVIEW_TILE;
          const int r1 = min((max(ra.y, max(rb.y, rc.y)) - 128) >> 8, ty * HGS_MESHVIEW_TILE + HGS_MESHVIEW_TILE - 1) - ty * HGS_MESHVIEW_TILE;
          if (c0 <= c1 && r0 <= r1)
            T.mask = (((2u << c1) - 1u) & ~((1u << c0) - 1u)) | ((((2u << r1) - 1u) & ~((1u << r0) - 1u)) << 16);
          T.zw[0] = __int_as_float(ra.z); T.zw[1] = __int_as_float(rb.z); T.zw[2] = __int_as_float(rc.z);
          T.iw[0] = __int_as_float(ra.w); T.iw[1] = __int_as_float(rb.w); T.iw[2] = __int_as_float(rc.w);
        }
      }
      sTri[tid] = T;          // (a triangle that is not drawn has an empty mask: no wave takes it up)
    }
    __syncthreads();
    // 64 triangles at a time: each lane asks whether ITS triangle's box meets the wave's four rows, and the wave then walks
    // the ones that do (most triangles of a body are a few pixels wide: a wave passes by most of a tile's list)
    for (int c = 0; c < m; c += 64) {
      const uint32_t mine = c + lane < m ? sTri[c + lane].mask : 0u;
      unsigned long long todo = __ballot((mine & wave_rows) != 0u && (mine & 0xffffu) != 0u);
      while (todo) {
        const int k = c + (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const MvTri T = sTri[k];
        const uint32_t in_box = T.mask & lane_mask;
        if (!(in_box & 0xffffu) || !(in_box >> 16)) continue;
        const long long E0 = T.E0 + ((long long)dx * T.st[0] + (long long)dy * T.st[1]);
        const long long E1 = T.E1 + ((long long)dx * T.st[2] + (long long)dy * T.st[3]);
        const long long E2 = T.A - E0 - E1;
        if (((E0 - (T.bias & 1)) | (E1 - ((T.bias >> 1) & 1)) | (E2 - ((T.bias >> 2) & 1))) < 0) continue;
        const float b0 = (float)E0 * T.ia, b1 = (float)E1 * T.ia, b2 = (float)E2 * T.ia;
        const float z = (b0 * T.zw[0] + b1 * T.zw[1]) + b2 * T.zw[2];
        if (!(z >= -1.0f && z <= 1.0f)) continue;
        if (z < bz || (z == bz && T.id < bid)) {
          bz = z; bid = T.id;
          bp0 = b0 * T.iw[0]; bp1 = b1 * T.iw[1]; bp2 = b2 * T.iw[2];
        }
      }
    }
  }
  if (!live) return;
  const bool hit = bid != 0x7fffffff;
  float u = 0.0f, v = 0.0f;
  if (hit) {
    const float d = (bp0 + bp1) + bp2;
    u = __fdiv_rn(bp0, d); v = __fdiv_rn(bp1, d);
  }
  const size_t pix = ((size_t)b * a.H + py) * a.W + px;
  if (a.rast) reinterpret_cast<float4*>(a.rast)[pix] = hit ? make_float4(u, v, bz, (float)(bid + 1)) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (a.image) mv_shade(a, b, hit ? bid : -1, u, v, a.background, a.shade_normals != 0, a.image + pix * a.C);
}

extern "C" __global__ void __launch_bounds__(HGS_MV_THREADS)
hgs_k_mv_interpolate(const hgs_meshview_args a) {
  const long long pix = (long long)blockIdx.x * HGS_MV_THREADS + threadIdx.x;
  const long long per_view = (long long)a.H * a.W;
  if (pix >= per_view * a.B) return;
  const float4 r = reinterpret_cast<const float4*>(a.rast_in)[pix];
  int face = -1;
  if (r.w >= 1.0f && r.w <= (float)a.F) face = (int)r.w - 1;      // (a NaN fails both)
  mv_shade(a, (int)(pix / per_view), face, r.x, r.y, 0.0f, false, a.image + (size_t)pix * a.C);
}
