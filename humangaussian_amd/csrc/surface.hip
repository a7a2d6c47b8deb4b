// surface.hip - area-uniform samples of a triangle mesh and the initial Gaussians built from a point cloud: the first stage
// of a run, `Skeleton.sample_smplx_points` (trimesh.sample.sample_surface on the CPU: threestudio/utils/poser.py:225-231)
// and the tensor chain of `GaussianModel.create_from_pcd` (gaussiansplatting/scene/gaussian_model.py:124-147).
//
// Contract: include/hgs_rast.h, hgs_surface_* and hgs_init_gaussians; tests/surface_sample_reference.py restates it in numpy.
//
//   table    cdf[0 .. F] fp64, cdf[0] = 0, cdf[k] = area of faces 0 .. k-1 summed in face order (the double instance of
//            gridscan.h's scan: left-to-right sums, so the table never decreases and a face of area 0 repeats the entry in
//            front of it).  Three launches of 1024 threads: areas + block totals, carry, prefix.
//   sample   one thread per sample, one launch: Philox4x32-10 of the sample's global index -> t in [0, A) -> the largest k
//            with cdf[k] <= t.  Every 2^s-th entry of the table is staged in LDS (s = 4 up to 32 767 faces: 10.2 KB at
//            SMPL-X's 20 908); the search there leaves a window of 2^s entries, halved from global memory (the table stays
//            in L2) down to 16 entries = one 128-byte line, which the lane loads whole and counts.  Integer barycentric
//            coordinates (trimesh's fold), the point with hgs_k_reanchor's expression.  points and uvw leave through LDS,
//            so that a wave stores 256 contiguous bytes per instruction.  No atomics, no scratch memory.
//   init     one thread per output float of a row (dc, rest, scaling, rotation, opacity, max_radii2D), one launch.
#include "hgs_common.h"

#define HGS_SURF_THREADS 256
#define HGS_SURF_COARSE_MAX 2048                         // table entries staged in LDS (16 KB)
#define HGS_SURF_WINDOW 16                               // table entries a lane counts at the end (128 bytes)

struct SurfInfo {                                        // = hgs_surface_info
  double area;
  uint32_t num_positive;
  uint32_t reserved;
};

// fp64 area of face f from its fp32 vertices; 0 for an index outside [0, V) (nothing is read then) and for a non-finite area
__device__ __forceinline__ double surf_face_area(int V, const float* __restrict__ vtx, const int32_t* __restrict__ faces, uint32_t f) {
  const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return 0.0;
  const double ax = vtx[3 * (size_t)i0], ay = vtx[3 * (size_t)i0 + 1], az = vtx[3 * (size_t)i0 + 2];
  const double bx = vtx[3 * (size_t)i1], by = vtx[3 * (size_t)i1 + 1], bz = vtx[3 * (size_t)i1 + 2];
  const double cx = vtx[3 * (size_t)i2], cy = vtx[3 * (size_t)i2 + 1], cz = vtx[3 * (size_t)i2 + 2];
  const double e1x = bx - ax, e1y = by - ay, e1z = bz - az;
  const double e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
  return isfinite(area) ? area : 0.0;
}

// cdf[i] = area of face i (i < F), cdf[F] = 0: the addends, in place of the table; bsum[block] = the block's total
extern "C" __global__ void __launch_bounds__(HGS_SCAN_BLOCK)
hgs_k_surface_area(int V, uint32_t F, const float* __restrict__ vtx, const int32_t* __restrict__ faces, double* cdf,
                   double* __restrict__ bsum) {
  const uint32_t i = blockIdx.x * HGS_SCAN_BLOCK + threadIdx.x;
  if (i <= F) cdf[i] = i < F ? surf_face_area(V, vtx, faces, i) : 0.0;      // (read back by this thread alone)
  hgs_scan_totals(F + 1u, (const double*)cdf, bsum);
}

extern "C" __global__ void __launch_bounds__(HGS_SCAN_BLOCK)
hgs_k_surface_carry(uint32_t nb, double* bsum) {
  hgs_scan_carry(nb, (const double*)bsum, bsum);
}

// cdf[i] = the sum of the areas in front of face i; the thread of i == F holds the whole area.  The faces of positive
// area are counted with one integer atomic per wave (info is zeroed in front of the chain).
extern "C" __global__ void __launch_bounds__(HGS_SCAN_BLOCK)
hgs_k_surface_prefix(uint32_t F, double* cdf, const double* __restrict__ bsum, SurfInfo* __restrict__ info) {
  uint32_t i;
  double ex, raw;
  const bool live = hgs_scan_prefix(F + 1u, (const double*)cdf, bsum, i, ex, raw);
  if (live) cdf[i] = ex;
  if (live && i == F) info->area = ex;
  const unsigned long long pos = __ballot(live && raw > 0.0);
  if ((threadIdx.x & 63) == 0 && pos) atomicAdd(&info->num_positive, (uint32_t)__popcll(pos));
}

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11) ---------------------------------
__device__ __forceinline__ void surf_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                            uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

struct SurfSampleArgs {
  int32_t V, F;
  int32_t shift, ncoarse;            // every 2^shift-th table entry is staged: ncoarse = ceil((F + 1) / 2^shift) of them
  const float* vtx;
  const int32_t* faces;
  const double* cdf;
  unsigned long long N, offset;
  uint32_t seed_lo, seed_hi;
  float* points;
  int32_t* face;
  float* uvw;
};

extern "C" __global__ void __launch_bounds__(HGS_SURF_THREADS)
hgs_k_surface_sample(SurfSampleArgs a) {
  __shared__ double coarse[HGS_SURF_COARSE_MAX];
  __shared__ float out_p[3 * HGS_SURF_THREADS], out_w[3 * HGS_SURF_THREADS];
  const int tid = threadIdx.x;
  const unsigned long long base = (unsigned long long)blockIdx.x * HGS_SURF_THREADS, i = base + tid;
  const bool live = i < a.N;
  const int F = a.F;
  const double A = F > 0 ? a.cdf[F] : 0.0;
  const bool usable = F > 0 && A > 0.0;                  // (uniform)
  if (usable)
    for (int m = tid; m < a.ncoarse; m += HGS_SURF_THREADS) coarse[m] = a.cdf[(size_t)m << a.shift];
  __syncthreads();

  int face = -1;
  float wu = 0.0f, wv = 0.0f, ww = 0.0f;
  float px = __builtin_nanf(""), py = px, pz = px;
  if (live && usable) {
    const unsigned long long g = a.offset + i;
    uint32_t x[4];
    surf_philox((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, a.seed_lo, a.seed_hi, x);
    const double u = ((double)(x[0] >> 5) * 67108864.0 + (double)(x[1] >> 6)) * 0x1.0p-53;
    const double t = u * A;
    // the largest staged entry <= t (entry 0 is 0 <= t)
    int lo = 0, hi = a.ncoarse;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (coarse[mid] <= t) lo = mid; else hi = mid;
    }
    // its window of 2^shift entries, halved down to HGS_SURF_WINDOW; an entry behind the table counts as > t
    int k0 = lo << a.shift;
    for (int width = 1 << a.shift; width > HGS_SURF_WINDOW; width >>= 1) {
      const int mid = k0 + (width >> 1);
      if (mid <= F && a.cdf[mid] <= t) k0 = mid;
    }
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < HGS_SURF_WINDOW; ++j) {
      const int k = k0 + j;
      const double c = k <= F ? a.cdf[k] : __builtin_inf();
      cnt += c <= t ? 1 : 0;
    }
    face = k0 + cnt - 1;                                 // = the number of k in 1 .. F with cdf[k] <= t
    face = face < 0 ? 0 : (face > F - 1 ? F - 1 : face); // (t < A = cdf[F]: never fires for a finite table)
    uint32_t k1 = x[2] >> 8, k2 = x[3] >> 8;
    if (k1 + k2 > (1u << 24)) { k1 = (1u << 24) - k1; k2 = (1u << 24) - k2; }
    wu = (float)((1u << 24) - k1 - k2) * 0x1.0p-24f; wv = (float)k1 * 0x1.0p-24f; ww = (float)k2 * 0x1.0p-24f;
    if (a.points) {
      const int i0 = a.faces[3 * (size_t)face], i1 = a.faces[3 * (size_t)face + 1], i2 = a.faces[3 * (size_t)face + 2];
      // (a face the search can reach has a positive area, hence indices inside [0, V); the test keeps a table that is
      //  not finite from reading outside the vertices)
      if ((unsigned)i0 < (unsigned)a.V && (unsigned)i1 < (unsigned)a.V && (unsigned)i2 < (unsigned)a.V) {
        const float ax = a.vtx[3 * (size_t)i0], ay = a.vtx[3 * (size_t)i0 + 1], az = a.vtx[3 * (size_t)i0 + 2];
        const float bx = a.vtx[3 * (size_t)i1], by = a.vtx[3 * (size_t)i1 + 1], bz = a.vtx[3 * (size_t)i1 + 2];
        const float cx = a.vtx[3 * (size_t)i2], cy = a.vtx[3 * (size_t)i2 + 1], cz = a.vtx[3 * (size_t)i2 + 2];
        px = (ax * wu + bx * wv) + cx * ww;              // hgs_k_reanchor's barycentric part
        py = (ay * wu + by * wv) + cy * ww;
        pz = (az * wu + bz * wv) + cz * ww;
      }
    }
  }
  if (live && a.face) a.face[i] = face;
  // points and uvw: the workgroup's 768 floats of each, stored in memory order
  out_p[3 * tid] = px; out_p[3 * tid + 1] = py; out_p[3 * tid + 2] = pz;
  out_w[3 * tid] = wu; out_w[3 * tid + 1] = wv; out_w[3 * tid + 2] = ww;
  __syncthreads();
  const unsigned long long rest = a.N - base;            // (base < N: the grid has ceil(N / 256) workgroups)
  const unsigned nfl = 3u * (unsigned)(rest < HGS_SURF_THREADS ? rest : HGS_SURF_THREADS);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const unsigned e = (unsigned)tid + (unsigned)j * HGS_SURF_THREADS;
    if (e < nfl) {
      if (a.points) a.points[3 * base + e] = out_p[e];
      if (a.uvw) a.uvw[3 * base + e] = out_w[e];
    }
  }
}

// ---- create_from_pcd's tensors (gaussian_model.py:127-147) -------------------------------------------------------------
struct InitGaussiansArgs {
  long long P;
  int32_t rest_floats;               // 3 (M - 1)
  float opacity;                     // log(0.1f / (1 - 0.1f)), rounded once on the host
  const float* colors;               // or nullptr: 0.5
  const float* dist2;
  float* features_dc;
  float* features_rest;
  float* scaling;
  float* rotation;
  float* opacity_out;
  float* max_radii2D;
};

// thread e -> float e of the row-major [P][12 + rest_floats] image of all outputs:
// columns 0-2 dc | 3-5 scaling | 6-9 rotation | 10 opacity | 11 max_radii2D | 12.. rest
extern "C" __global__ void __launch_bounds__(256)
hgs_k_init_gaussians(InitGaussiansArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  const int W = 12 + a.rest_floats;
  if (e >= a.P * W) return;
  const long long p = e / W;
  const int c = (int)(e - p * W);
  if (c < 3) {
    if (a.features_dc) a.features_dc[3 * p + c] = ((a.colors ? a.colors[3 * p + c] : 0.5f) - 0.5f) / 0.28209479177387814f;
  } else if (c < 6) {
    if (a.scaling) {
      const float d = a.dist2[p];                        // (clamp_min keeps a NaN; fmaxf would drop it)
      a.scaling[3 * p + (c - 3)] = logf(sqrtf(d < 0.0000001f ? 0.0000001f : d));
    }
  } else if (c < 10) {
    if (a.rotation) a.rotation[4 * p + (c - 6)] = c == 6 ? 1.0f : 0.0f;
  } else if (c == 10) {
    if (a.opacity_out) a.opacity_out[p] = a.opacity;
  } else if (c == 11) {
    if (a.max_radii2D) a.max_radii2D[p] = 0.0f;
  } else {
    if (a.features_rest) a.features_rest[(long long)a.rest_floats * p + (c - 12)] = 0.0f;
  }
}
