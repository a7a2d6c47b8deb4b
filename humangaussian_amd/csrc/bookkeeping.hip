// bookkeeping.hip - the per-step bookkeeping either side of the rasterize hot path (SURVEY.md 8(f)-3,
// 8(f)-4), as single-pass HIP kernels.  All of it is HBM-bound elementwise / gather work: one
// coalesced pass over the per-Gaussian arrays, no atomics except the three mask counters.
//
// Reference code replaced (torch elementwise kernels launched from Python, a dozen per call):
//   densification statistics   threestudio/systems/GaussianDreamer.py:253-256,289,385-391 +
//                              gaussiansplatting/scene/gaussian_model.py:434-438
//   clone / split / prune masks gaussian_model.py:359-438 (densify_and_clone, densify_and_split,
//                              densify_and_prune, prune_only)
//   row compaction             gaussian_model.py:283-337 (_prune_optimizer: boolean-mask indexing of
//                              every parameter tensor and of both Adam moments)
//   re-anchoring               animation.py:384-403 (numpy on the CPU + H2D per frame)
#include "hgs_common.h"

// ---- densification statistics of one training step (B views) -------------------------------------
// Per Gaussian: radii_max = max over views, visible = radii_max > 0 (and keep[i] when given: the
// reference masks near-hand points), g = sum over views (view order) of dL/dmeans2D, and for
// visible Gaussians  max_radii2D = max(max_radii2D, radii_max),  accum += |g.xy|,  denom += 1.
extern "C" __global__ void __launch_bounds__(256)
hgs_k_densify_stats(int B, int P, const float* __restrict__ g2d, const int32_t* __restrict__ radii,
                    const uint8_t* __restrict__ keep, float* __restrict__ accum, float* __restrict__ denom,
                    float* __restrict__ max_radii2D, int32_t* __restrict__ radii_max_out,
                    uint8_t* __restrict__ visible_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  int rmax = 0;
  float gx = 0.f, gy = 0.f;
  for (int b = 0; b < B; ++b) {
    rmax = max(rmax, radii[(size_t)b * P + i]);
    const float* g = g2d + ((size_t)b * P + i) * 3;
    gx += g[0];
    gy += g[1];
  }
  const bool vis = rmax > 0 && (!keep || keep[i]);
  if (vis) {
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)rmax);
    accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
  }
  if (radii_max_out) radii_max_out[i] = rmax;
  if (visible_out) visible_out[i] = vis ? 1 : 0;
}

// ---- clone / split / prune masks ---------------------------------------------------------------
// grad = accum / denom (NaN -> 0).  big = max_k scale_k > percent_dense * extent.
//   clone = grad >= thr && !big         (densify_and_clone)
//   split = grad >= thr &&  big         (densify_and_split)
//   prune = opacity < min_opacity || (max_screen_size > 0 && (max_radii2D > max_screen_size ||
//           max scale > 0.1 * extent)) || (size_thresh > 0 && max scale > size_thresh)   (densify_and_prune / prune_only)
// scales / opacity arrive raw (log-scale, logit) when the flags say so: the activations are fused.
// counts[0..2] += number of set clone / split / prune bits (the host sizes its tensors with them).
extern "C" __global__ void __launch_bounds__(256)
hgs_k_densify_masks(int P, const float* __restrict__ accum, const float* __restrict__ denom,
                    const float* __restrict__ scales, int scales_are_log, const float* __restrict__ opacity,
                    int opacity_is_logit, const float* __restrict__ max_radii2D, float grad_threshold,
                    float percent_dense, float extent, float min_opacity, float max_screen_size,
                    float size_thresh, uint8_t* __restrict__ clone, uint8_t* __restrict__ split,
                    uint8_t* __restrict__ prune, uint32_t* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool c = false, s = false, p = false;
  if (i < P) {
    float g = accum[i] / denom[i];
    if (g != g) g = 0.0f;
    float s0 = scales[3 * i + 0], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    if (scales_are_log) { s0 = expf(s0); s1 = expf(s1); s2 = expf(s2); }
    const float smax = fmaxf(s0, fmaxf(s1, s2));
    float op = opacity[i];
    if (opacity_is_logit) op = 1.0f / (1.0f + expf(-op));
    const bool big = smax > percent_dense * extent;
    c = (g >= grad_threshold) && !big;
    s = (g >= grad_threshold) && big;
    p = op < min_opacity;
    if (max_screen_size > 0.0f) p = p || (max_radii2D[i] > max_screen_size) || (smax > 0.1f * extent);
    if (size_thresh > 0.0f) p = p || (smax > size_thresh);
    if (clone) clone[i] = c;
    if (split) split[i] = s;
    if (prune) prune[i] = p;
  }
  if (counts) {
    const unsigned long long bc = __ballot(c), bs = __ballot(s), bp = __ballot(p);
    if ((threadIdx.x & 63) == 0) {
      if (bc) atomicAdd(&counts[0], (uint32_t)__popcll(bc));
      if (bs) atomicAdd(&counts[1], (uint32_t)__popcll(bs));
      if (bp) atomicAdd(&counts[2], (uint32_t)__popcll(bp));
    }
  }
}

// ---- stable row compaction (prune every parameter tensor and both Adam moments) ---------------------
// pass 1: per 1024-row block popcount of keep[]; pass 2 (one workgroup): exclusive scan of the block
// counts; pass 3: rows of the kept indices move to their compacted position, order preserved.
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_keep_count(int P, const uint8_t* __restrict__ keep, uint32_t* __restrict__ block_count) {
  __shared__ uint32_t wsum[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const unsigned long long b = __ballot(i < P && keep[i]);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int k = 0; k < 16; ++k) t += wsum[k];
    block_count[blockIdx.x] = t;
  }
}

extern "C" __global__ void __launch_bounds__(1024)
hgs_k_keep_scan(int nblocks, uint32_t* __restrict__ block_count, uint32_t* __restrict__ total) {
  const uint32_t kept = hgs_scan_carry((uint32_t)nblocks, block_count, block_count);      // gridscan.h
  if (threadIdx.x == 0) *total = kept;
}

// dst row of kept source row i = block base + rank of i among the kept rows of its block
extern "C" __global__ void __launch_bounds__(1024)
hgs_k_keep_index(int P, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ block_base,
                 int32_t* __restrict__ src_of_dst) {
  __shared__ uint32_t wsum[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const bool k = i < P && keep[i];
  const unsigned long long b = __ballot(k);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) wsum[w] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t base = block_base[blockIdx.x];
  for (int q = 0; q < w; ++q) base += wsum[q];
  if (k) {
    const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    src_of_dst[base + r] = i;
  }
}

// dst[j][0..row_floats) = src[src_of_dst[j]][..]; one thread per float, coalesced on the output
extern "C" __global__ void __launch_bounds__(256)
hgs_k_gather_rows(long long n_out_floats, int row_floats, const int32_t* __restrict__ src_of_dst,
                  const float* __restrict__ src, float* __restrict__ dst) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out_floats) return;
  const long long j = e / row_floats;
  const int c = (int)(e - j * row_floats);
  dst[e] = src[(long long)src_of_dst[j] * row_floats + c];
}

// ---- re-anchoring of the Gaussians on a posed mesh (animation.py:384-403) -----------------------------
// xyz[i] = u*v0 + v*v1 + w*v2 + dist[i] * n,  n = cross(v1-v0, v2-v0) / (|.| + 1e-20), (v0,v1,v2) = the
// vertices of face mapping_face[i].
extern "C" __global__ void __launch_bounds__(256)
hgs_k_reanchor(int P, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
               const int32_t* __restrict__ mapping_face, const float* __restrict__ mapping_uvw,
               const float* __restrict__ mapping_dist, float* __restrict__ xyz) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int f = mapping_face[i];
  const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  const float ax = vertices[3 * i0], ay = vertices[3 * i0 + 1], az = vertices[3 * i0 + 2];
  const float bx = vertices[3 * i1], by = vertices[3 * i1 + 1], bz = vertices[3 * i1 + 2];
  const float cx = vertices[3 * i2], cy = vertices[3 * i2 + 1], cz = vertices[3 * i2 + 2];
  const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
  const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
  float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float inv = 1.0f / (sqrtf(nx * nx + ny * ny + nz * nz) + 1e-20f);
  nx *= inv; ny *= inv; nz *= inv;
  const float u = mapping_uvw[3 * i], vv = mapping_uvw[3 * i + 1], w = mapping_uvw[3 * i + 2];
  const float d = mapping_dist[i];
  xyz[3 * i + 0] = (ax * u + bx * vv + cx * w) + d * nx;
  xyz[3 * i + 1] = (ay * u + by * vv + cy * w) + d * ny;
  xyz[3 * i + 2] = (az * u + bz * vv + cz * w) + d * nz;
}

// ---- re-anchoring that also carries the rotations (opt-in; include/hgs_rast.h: hgs_reanchor_rot) -----------------
// The frame of face (a, b, c):  e1 = (b-a)/|b-a|,  n = (b-a)x(c-a)/|.|,  e2 = n x e1,  F = [e1 e2 n] (columns);  r = a unit
// quaternion (w,x,y,z) of F, taken from the largest of the four diagonal terms 1+-F00+-F11+-F22 (each is four times a squared
// component, their sum is 4: the largest is >= 1, so no branch divides by a small number).  r = (1,0,0,0) where |b-a|^2 or
// |(b-a)x(c-a)|^2 is below 1e-30 or not finite.  Every operation is rounded to fp32 in the order written (no contraction);
// tests/reanchor_rot_reference.py restates it operation by operation.
//   BIND:  rot_out = conj(r) (x) rot_in   (once per avatar, at the rest mesh; xyz is written only where given)
//   else:  rot_out = r (x) rot_in,  xyz[i] = hgs_k_reanchor's expressions in hgs_k_reanchor's order (the same bits)
// (x) is the Hamilton product.  One thread per Gaussian, the three vertices loaded once; no LDS, no atomics, no arrays (a
// quaternion picked by index would live in scratch: the four candidates are picked by selects).
template <bool BIND>
__device__ __forceinline__ void hgs_reanchor_rot_body(int P, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                      const int32_t* __restrict__ mapping_face,
                                                      const float* __restrict__ mapping_uvw,
                                                      const float* __restrict__ mapping_dist, const float* __restrict__ rot_in,
                                                      float* __restrict__ xyz, float* __restrict__ rot_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const int f = mapping_face[i];
  const int i0 = faces[3 * f + 0], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  const float ax = vertices[3 * i0], ay = vertices[3 * i0 + 1], az = vertices[3 * i0 + 2];
  const float bx = vertices[3 * i1], by = vertices[3 * i1 + 1], bz = vertices[3 * i1 + 2];
  const float cx = vertices[3 * i2], cy = vertices[3 * i2 + 1], cz = vertices[3 * i2 + 2];
  const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
  const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
  const float mx = e1y * e2z - e1z * e2y, my = e1z * e2x - e1x * e2z, mz = e1x * e2y - e1y * e2x;
  const float mm = mx * mx + my * my + mz * mz;
  if (!BIND || xyz) {                                           // hgs_k_reanchor, expression for expression
    const float inv = 1.0f / (sqrtf(mm) + 1e-20f);
    const float nx = mx * inv, ny = my * inv, nz = mz * inv;
    const float u = mapping_uvw[3 * i], vv = mapping_uvw[3 * i + 1], w = mapping_uvw[3 * i + 2];
    const float d = mapping_dist[i];
    xyz[3 * i + 0] = (ax * u + bx * vv + cx * w) + d * nx;
    xyz[3 * i + 1] = (ay * u + by * vv + cy * w) + d * ny;
    xyz[3 * i + 2] = (az * u + bz * vv + cz * w) + d * nz;
  }
  const float ll = e1x * e1x + e1y * e1y + e1z * e1z;
  // (a NaN fails both comparisons of its line: not finite -> the identity)
  const bool sound = ll >= 1e-30f && ll <= 3.402823466e38f && mm >= 1e-30f && mm <= 3.402823466e38f;
  float rw = 1.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f;
  if (sound) {
    const float l = sqrtf(ll), m = sqrtf(mm);
    const float f00 = e1x / l, f10 = e1y / l, f20 = e1z / l;                       // e1
    const float f02 = mx / m, f12 = my / m, f22 = mz / m;                          // n
    const float f01 = f12 * f20 - f22 * f10, f11 = f22 * f00 - f02 * f20, f21 = f02 * f10 - f12 * f00;   // e2 = n x e1
    const float tw = ((1.0f + f00) + f11) + f22, tx = ((1.0f + f00) - f11) - f22;
    const float ty = ((1.0f - f00) + f11) - f22, tz = ((1.0f - f00) - f11) + f22;
    const bool pw = tw >= tx && tw >= ty && tw >= tz;
    const bool px = !pw && tx >= ty && tx >= tz;
    const bool py = !pw && !px && ty >= tz;
    const float t = pw ? tw : (px ? tx : (py ? ty : tz));
    const float s = sqrtf(t);
    const float big = 0.5f * s, h = 0.5f / s;
    const float dw = f21 - f12, dy = f02 - f20, dz = f10 - f01;                   // 4 w x, 4 w y, 4 w z
    const float sxy = f01 + f10, sxz = f02 + f20, syz = f12 + f21;                // 4 x y, 4 x z, 4 y z
    rw = pw ? big : (px ? dw : (py ? dy : dz)) * h;
    rx = px ? big : (pw ? dw : (py ? sxy : sxz)) * h;
    ry = py ? big : (pw ? dy : (px ? sxy : syz)) * h;
    rz = (pw || px || py) ? (pw ? dz : (px ? sxz : syz)) * h : big;
  }
  if (BIND) { rx = -rx; ry = -ry; rz = -rz; }
  const float qw = rot_in[4 * i], qx = rot_in[4 * i + 1], qy = rot_in[4 * i + 2], qz = rot_in[4 * i + 3];
  rot_out[4 * i + 0] = ((rw * qw - rx * qx) - ry * qy) - rz * qz;
  rot_out[4 * i + 1] = ((rw * qx + rx * qw) + ry * qz) - rz * qy;
  rot_out[4 * i + 2] = ((rw * qy - rx * qz) + ry * qw) + rz * qx;
  rot_out[4 * i + 3] = ((rw * qz + rx * qy) - ry * qx) + rz * qw;
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_reanchor_rot_bind(int P, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                        const int32_t* __restrict__ mapping_face, const float* __restrict__ mapping_uvw,
                        const float* __restrict__ mapping_dist, const float* __restrict__ rot_in, float* __restrict__ xyz,
                        float* __restrict__ rot_out) {
  hgs_reanchor_rot_body<true>(P, vertices, faces, mapping_face, mapping_uvw, mapping_dist, rot_in, xyz, rot_out);
}

extern "C" __global__ void __launch_bounds__(256)
hgs_k_reanchor_rot_pose(int P, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                        const int32_t* __restrict__ mapping_face, const float* __restrict__ mapping_uvw,
                        const float* __restrict__ mapping_dist, const float* __restrict__ rot_in, float* __restrict__ xyz,
                        float* __restrict__ rot_out) {
  hgs_reanchor_rot_body<false>(P, vertices, faces, mapping_face, mapping_uvw, mapping_dist, rot_in, xyz, rot_out);
}
