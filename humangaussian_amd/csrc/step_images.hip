// step_images.hip - the stretch between the batched render and the diffusion guidance: the two 3-channel images the
// guidance is handed (bilinear resize of the colour, and of the per-view normalised depth) and the two opacity losses,
// forward and backward in three launches each (include/hgs_rast.h: hgs_step_images_* states the formulas).
//
// Reference code replaced: threestudio/systems/GaussianDreamer.py:285-302, :330-333, :359-366 and
// threestudio/models/guidance/dual_branch_guidance.py:762-770 - about 20 torch kernels forward and more backward.
//
// Two decompositions:
//   reductions  a view's H W depth pixels are cut into CHUNKS of HGS_SI_PIXELS_PER_WORKGROUP (256 threads x 4 pixels, one
//               16-byte load per lane); a view gets P = min(chunks, HGS_SI_PARTIALS_PER_VIEW) workgroups, workgroup p
//               takes chunks p, p + P, ... (256: 2048 workgroups for 8 views of 1024 x 1024; with 64 the step of
//               tools/step_images_bench.py took 192 instead of 183 us).  Every workgroup leaves ONE partial per sum
//               (its threads add their pixels in order, then a fixed tree over the lanes and the four waves); the
//               partials meet in a one-workgroup launch in a fixed order in fp64.  No floating-point atomics, no
//               integer ones either: tie counts are partials too.
//   images      a thread owns four consecutive pixels of one row of one plane (16-byte store, or 8-byte for fp16), planes
//               are (view, r / g / b / depth).  The forward gathers 2 x 2 inputs per output; the backward gathers, per
//               INPUT pixel, the outputs that read it (at most two per axis when downsampling; five candidates are
//               tested with the forward's own fp32 index arithmetic so a rounding of `src` cannot lose one).  Exact 2:1
//               with W % 8 == 0 takes 16-byte loads of two rows; the arithmetic, and so every bit, is that of the gather.
//
// hgs_k_si_minmax     F1  per-workgroup min / max of the depth
// hgs_k_si_forward    F2  workgroups [0, B P): loss and tie-count partials (need g: all partials of F1);
//                         the rest: the image planes (the depth plane needs its view's partials)
// hgs_k_si_finish     F3  one workgroup: depth_min / max / global max, tie counts, the two losses
// hgs_k_si_bwd_sums   B1  per-workgroup partials of the three tie-share sums
// hgs_k_si_bwd_finish B2  one workgroup: the shares dL/ddmin / count, dL/ddmax / count, dL/dg / count
// hgs_k_si_bwd_write  B3  dL/drender and dL/ddepth, every element written once
#include "hgs_common.h"
#include <hip/hip_fp16.h>

#define HGS_SI_THREADS 256
#define HGS_SI_WAVES (HGS_SI_THREADS / 64)
static_assert(HGS_SI_PIXELS_PER_WORKGROUP == HGS_SI_THREADS * HGS_SI_PIXELS_PER_THREAD, "a chunk is one 16-byte access per lane");

// partials per view, chunks per view
__host__ __device__ __forceinline__ int hgs_si_chunks(int H, int W) {
  return (int)(((long long)H * W + HGS_SI_PIXELS_PER_WORKGROUP - 1) / HGS_SI_PIXELS_PER_WORKGROUP);
}
__host__ __device__ __forceinline__ int hgs_si_partials(int H, int W) {
  const int c = hgs_si_chunks(H, W);
  return c < HGS_SI_PARTIALS_PER_VIEW ? c : HGS_SI_PARTIALS_PER_VIEW;
}

// workspace, in 4-byte words, n = B P.  Forward: pmin, pmax, loss_s, loss_o (float), cmin, cmax, cg (uint32).
// Backward: s1, s2, sg (float), then the shares: [b] min, [B + b] max, [2 B] global.
#define HGS_SI_WS_FWD_WORDS 7
#define HGS_SI_WS_BWD_WORDS 3

struct SiAxis { int i0, i1; float w0, w1; };

// torch's align_corners=False source index of output `dst` (area_pixel_compute_source_index, guard_index_and_lambda)
__device__ __forceinline__ SiAxis si_axis(int dst, int in, float scale) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  SiAxis a;
  a.i0 = min((int)src, in - 1);
  a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
  a.w1 = fminf(fmaxf(src - (float)a.i0, 0.0f), 1.0f);
  a.w0 = 1.0f - a.w1;
  return a;
}

// the weight with which output `o` reads input `i` (the transpose of the resize), 0 if it does not
__device__ __forceinline__ float si_weight_t(int i, int o, int in, int out, float scale) {
  if (o < 0 || o >= out) return 0.0f;
  const SiAxis a = si_axis(o, in, scale);
  return (a.i0 == i ? a.w0 : 0.0f) + (a.i1 == i ? a.w1 : 0.0f);
}

// first of the five candidate outputs of input i: floor of the exact output coordinate ((2 i + 1) out - in) / (2 in), - 2
__device__ __forceinline__ int si_first_candidate(int i, int in, int out) {
  const long long num = (2ll * i + 1) * out - in, den = 2ll * in;
  const long long f = num >= 0 ? num / den : -((-num + den - 1) / den);
  return (int)f - 2;
}

__device__ __forceinline__ float si_load_grad(const void* p, size_t i, int half_images) {
  return half_images ? __half2float(static_cast<const __half*>(p)[i]) : static_cast<const float*>(p)[i];
}

// ---- workgroup reductions in a fixed order: lanes by halving strides, then the four waves in order ----
static_assert(HGS_SI_WAVES == 4, "si_block_reduce combines four waves");
template <typename T, typename Op>
__device__ __forceinline__ T si_block_reduce(T v, T* lds, Op op) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = op(v, __shfl_down(v, s, 64));
  __syncthreads();                 // protect lds from a previous use
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(op(lds[0], lds[1]), lds[2]), lds[3]);
}
template <typename T>
__device__ __forceinline__ T si_block_sum(T v, T* lds) { return si_block_reduce(v, lds, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ float si_block_min(float v, float* lds) { return si_block_reduce(v, lds, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float si_block_max(float v, float* lds) { return si_block_reduce(v, lds, [](float a, float b) { return fmaxf(a, b); }); }

// the four pixels of a thread in chunk c of view b: n of them are inside the view (0..4)
__device__ __forceinline__ int si_chunk_load(const float* __restrict__ plane, long long HW, int c, float v[4], long long& first) {
  first = (long long)c * HGS_SI_PIXELS_PER_WORKGROUP + (long long)threadIdx.x * HGS_SI_PIXELS_PER_THREAD;
  const long long left = HW - first;
  const int n = left >= HGS_SI_PIXELS_PER_THREAD ? HGS_SI_PIXELS_PER_THREAD : (left > 0 ? (int)left : 0);
  if (n == HGS_SI_PIXELS_PER_THREAD && (HW & 3) == 0) {      // every view then starts on a 16-byte boundary
    const float4 q = *reinterpret_cast<const float4*>(plane + first);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < HGS_SI_PIXELS_PER_THREAD; ++k) v[k] = k < n ? plane[first + k] : 0.0f;
  }
  return n;
}

extern "C" __global__ void __launch_bounds__(HGS_SI_THREADS)
hgs_k_si_minmax(const hgs_step_images_args a) {
  __shared__ float red[HGS_SI_WAVES];
  const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  const long long HW = (long long)a.H * a.W;
  const float* __restrict__ plane = a.depth + (size_t)b * HW;
  const int chunks = hgs_si_chunks(a.H, a.W);
  float lo = INFINITY, hi = -INFINITY;
  for (int c = p; c < chunks; c += P) {
    float v[4];
    long long first;
    const int n = si_chunk_load(plane, HW, c, v, first);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) { lo = fminf(lo, v[k]); hi = fmaxf(hi, v[k]); }
  }
  lo = si_block_min(lo, red);
  hi = si_block_max(hi, red);
  if (threadIdx.x == 0) {
    float* ws = static_cast<float*>(a.workspace);
    const size_t n = (size_t)a.B * P;
    ws[(size_t)b * P + p] = lo;
    ws[n + (size_t)b * P + p] = hi;
  }
}

// min and max of view b, and (all = true) the max over every view, from the partials of F1: exact in any order
__device__ __forceinline__ void si_view_stats(const hgs_step_images_args& a, int b, int P, bool all, float* red,
                                              float& dmin, float& dmax, float& g) {
  const float* ws = static_cast<const float*>(a.workspace);
  const size_t n = (size_t)a.B * P;
  float lo = INFINITY, hi = -INFINITY, gg = -INFINITY;
  for (int i = threadIdx.x; i < P; i += HGS_SI_THREADS) {
    lo = fminf(lo, ws[(size_t)b * P + i]);
    hi = fmaxf(hi, ws[n + (size_t)b * P + i]);
  }
  if (all)
    for (size_t i = threadIdx.x; i < n; i += HGS_SI_THREADS) gg = fmaxf(gg, ws[n + i]);
  dmin = si_block_min(lo, red);
  dmax = si_block_max(hi, red);
  g = all ? si_block_max(gg, red) : 0.0f;
}

__device__ __forceinline__ void si_store4(void* out, size_t i, const float r[4], int n, bool vec, int half_images) {
  if (half_images) {
    __half* o = static_cast<__half*>(out) + i;
    if (vec) {
      union { __half h[4]; uint2 u; } pk;
#pragma unroll
      for (int k = 0; k < 4; ++k) pk.h[k] = __float2half_rn(r[k]);
      *reinterpret_cast<uint2*>(o) = pk.u;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) o[k] = __float2half_rn(r[k]);
    }
  } else {
    float* o = static_cast<float*>(out) + i;
    if (vec) {
      *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) o[k] = r[k];
    }
  }
}

extern "C" __global__ void __launch_bounds__(HGS_SI_THREADS)
hgs_k_si_forward(const hgs_step_images_args a, const int P, const int blocks_per_plane) {
  __shared__ float red[HGS_SI_WAVES];
  __shared__ uint32_t redu[HGS_SI_WAVES];
  const long long HW = (long long)a.H * a.W;
  const size_t n = (size_t)a.B * P;
  float* ws = static_cast<float*>(a.workspace);

  if (blockIdx.x < n) {
    // ---- loss and tie-count partials of (view b, partial p) ----
    const int b = blockIdx.x / P, p = blockIdx.x % P;
    float dmin, dmax, g;
    si_view_stats(a, b, P, true, red, dmin, dmax, g);
    const float s = g + 1e-5f;
    const float* __restrict__ plane = a.depth + (size_t)b * HW;
    const int chunks = hgs_si_chunks(a.H, a.W);
    float ls = 0.0f, lo = 0.0f;
    uint32_t cmin = 0, cmax = 0, cg = 0;
    for (int c = p; c < chunks; c += P) {
      float v[4];
      long long first;
      const int cnt = si_chunk_load(plane, HW, c, v, first);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          const float d = v[k];
          const float op = d / s;
          ls += sqrtf(op * op + 0.01f);
          const float x = fminf(fmaxf(op, 1e-3f), 1.0f - 1e-3f);
          // torch's binary_cross_entropy with the input as its own target (its -100 floor of the logs is never reached)
          lo += (x - 1.0f) * logf(1.0f - x) - x * logf(x);
          cmin += d == dmin;
          cmax += d == dmax;
          cg += d == g;
        }
      }
    }
    ls = si_block_sum(ls, red);
    lo = si_block_sum(lo, red);
    cmin = si_block_sum(cmin, redu);
    cmax = si_block_sum(cmax, redu);
    cg = si_block_sum(cg, redu);
    if (threadIdx.x == 0) {
      uint32_t* wu = static_cast<uint32_t*>(a.workspace);
      ws[2 * n + blockIdx.x] = ls;
      ws[3 * n + blockIdx.x] = lo;
      wu[4 * n + blockIdx.x] = cmin;
      wu[5 * n + blockIdx.x] = cmax;
      wu[6 * n + blockIdx.x] = cg;
    }
    return;
  }

  // ---- the image planes: plane = b * 4 + c, c = 3 is the depth ----
  const unsigned r = blockIdx.x - (unsigned)n;
  const int plane = r / blocks_per_plane, blk = r % blocks_per_plane;
  const int b = plane >> 2, ch = plane & 3;
  const bool is_depth = ch == 3;
  float dmin = 0.0f, rng = 1.0f;
  if (is_depth) {     // (uniform over the workgroup)
    float dmax, g;
    si_view_stats(a, b, P, false, red, dmin, dmax, g);
    rng = dmax - dmin + 1e-10f;
  }
  const int groups = (a.w + 3) >> 2;                       // threads per output row
  const long long t = (long long)blk * HGS_SI_THREADS + threadIdx.x;
  if (t >= (long long)groups * a.h) return;
  const int oy = (int)(t / groups), ox0 = (int)(t % groups) * 4;
  const int cnt = min(4, a.w - ox0);
  const float* __restrict__ src = is_depth ? a.depth + (size_t)b * HW : a.render + ((size_t)b * 3 + ch) * HW;
  const float sy = (float)a.H / (float)a.h, sx = (float)a.W / (float)a.w;
  const SiAxis ay = si_axis(oy, a.H, sy);
  const float* __restrict__ row0 = src + (size_t)ay.i0 * a.W;
  const float* __restrict__ row1 = src + (size_t)ay.i1 * a.W;
  float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (a.H == 2 * a.h && a.W == 2 * a.w && (a.W & 7) == 0) {
    // exact 2:1: outputs ox0 .. ox0 + 3 read inputs 2 ox0 .. 2 ox0 + 7 of rows 2 oy, 2 oy + 1 with weight 1/2 per axis
    const float4 p0 = *reinterpret_cast<const float4*>(row0 + 2 * ox0), p1 = *reinterpret_cast<const float4*>(row0 + 2 * ox0 + 4);
    const float4 q0 = *reinterpret_cast<const float4*>(row1 + 2 * ox0), q1 = *reinterpret_cast<const float4*>(row1 + 2 * ox0 + 4);
    float top[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
    float bot[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    if (is_depth) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { top[k] = (top[k] - dmin) / rng; bot[k] = (bot[k] - dmin) / rng; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      out[k] = 0.5f * (0.5f * top[2 * k] + 0.5f * top[2 * k + 1]) + 0.5f * (0.5f * bot[2 * k] + 0.5f * bot[2 * k + 1]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < cnt) {
        const SiAxis ax = si_axis(ox0 + k, a.W, sx);
        float v00 = row0[ax.i0], v01 = row0[ax.i1], v10 = row1[ax.i0], v11 = row1[ax.i1];
        if (is_depth) { v00 = (v00 - dmin) / rng; v01 = (v01 - dmin) / rng; v10 = (v10 - dmin) / rng; v11 = (v11 - dmin) / rng; }
        out[k] = ay.w0 * (ax.w0 * v00 + ax.w1 * v01) + ay.w1 * (ax.w0 * v10 + ax.w1 * v11);
      }
    }
  }
  const size_t hw = (size_t)a.h * a.w;
  const bool vec = (a.w & 3) == 0;
  const size_t at = (size_t)oy * a.w + ox0;
  if (is_depth) {
#pragma unroll
    for (int c = 0; c < 3; ++c) si_store4(a.depth_out, ((size_t)b * 3 + c) * hw + at, out, cnt, vec, a.half_images);
  } else {
    si_store4(a.rgb_out, ((size_t)b * 3 + ch) * hw + at, out, cnt, vec, a.half_images);
  }
}

extern "C" __global__ void __launch_bounds__(HGS_SI_THREADS)
hgs_k_si_finish(const hgs_step_images_args a, const int P) {
  __shared__ float red[HGS_SI_WAVES];
  __shared__ uint32_t redu[HGS_SI_WAVES];
  __shared__ double redd[HGS_SI_WAVES];
  const float* ws = static_cast<const float*>(a.workspace);
  const uint32_t* wu = static_cast<const uint32_t*>(a.workspace);
  const size_t n = (size_t)a.B * P;
  float g = -INFINITY;
  uint32_t cg = 0;
  for (int b = 0; b < a.B; ++b) {
    float lo = INFINITY, hi = -INFINITY;
    uint32_t cmin = 0, cmax = 0;
    for (int i = threadIdx.x; i < P; i += HGS_SI_THREADS) {
      const size_t at = (size_t)b * P + i;
      lo = fminf(lo, ws[at]);
      hi = fmaxf(hi, ws[n + at]);
      cmin += wu[4 * n + at];
      cmax += wu[5 * n + at];
      cg += wu[6 * n + at];
    }
    lo = si_block_min(lo, red);
    hi = si_block_max(hi, red);
    cmin = si_block_sum(cmin, redu);
    cmax = si_block_sum(cmax, redu);
    g = fmaxf(g, hi);
    if (threadIdx.x == 0) {
      a.depth_min[b] = lo;
      a.depth_max[b] = hi;
      a.tie_counts[b] = cmin;
      a.tie_counts[a.B + b] = cmax;
    }
  }
  cg = si_block_sum(cg, redu);
  double ls = 0.0, lo = 0.0;
  for (size_t i = threadIdx.x; i < n; i += HGS_SI_THREADS) { ls += (double)ws[2 * n + i]; lo += (double)ws[3 * n + i]; }
  ls = si_block_sum(ls, redd);
  lo = si_block_sum(lo, redd);
  if (threadIdx.x == 0) {
    const double N = (double)a.B * (double)a.H * (double)a.W;
    a.depth_global_max[0] = g;
    a.tie_counts[2 * a.B] = cg;
    a.loss_sparsity[0] = (float)(ls / N);
    a.loss_opaque[0] = (float)(lo / N);
  }
}

// ------------------------------------------------------------------------------------------------------------ backward

// dL/dnd of input pixel (y, x) of view b: the three channels of grad_depth through the transpose of the resize
__device__ __forceinline__ float si_gather_depth_grad(const hgs_step_images_args& a, int b, int y, int x, float sy, float sx) {
  const size_t hw = (size_t)a.h * a.w, base = (size_t)b * 3 * hw;
  if (a.H == 2 * a.h && a.W == 2 * a.w) {
    const size_t at = base + (size_t)(y >> 1) * a.w + (x >> 1);
    const float gs = (si_load_grad(a.grad_depth, at, a.half_images) + si_load_grad(a.grad_depth, at + hw, a.half_images)) +
                     si_load_grad(a.grad_depth, at + 2 * hw, a.half_images);
    return (0.5f * 0.5f) * gs;
  }
  const int fy = si_first_candidate(y, a.H, a.h), fx = si_first_candidate(x, a.W, a.w);
  float acc = 0.0f;
  for (int j = 0; j < 5; ++j) {
    const float wy = si_weight_t(y, fy + j, a.H, a.h, sy);
    if (wy == 0.0f) continue;
    for (int i = 0; i < 5; ++i) {
      const float wx = si_weight_t(x, fx + i, a.W, a.w, sx);
      if (wx == 0.0f) continue;
      const size_t at = base + (size_t)(fy + j) * a.w + (fx + i);
      const float gs = (si_load_grad(a.grad_depth, at, a.half_images) + si_load_grad(a.grad_depth, at + hw, a.half_images)) +
                       si_load_grad(a.grad_depth, at + 2 * hw, a.half_images);
      acc += (wy * wx) * gs;
    }
  }
  return acc;
}

// dL/dop of a pixel: the two losses (N = B H W)
__device__ __forceinline__ float si_dloss_dop(float op, float gls, float glo, float invN) {
  float r = gls * (op / sqrtf(op * op + 0.01f)) * invN;
  if (op >= 1e-3f && op <= 1.0f - 1e-3f) r += glo * (logf(1.0f - op) - logf(op)) * invN;
  return r;
}

extern "C" __global__ void __launch_bounds__(HGS_SI_THREADS)
hgs_k_si_bwd_sums(const hgs_step_images_args a) {
  __shared__ float red[HGS_SI_WAVES];
  const int b = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  const long long HW = (long long)a.H * a.W;
  const float* __restrict__ plane = a.depth + (size_t)b * HW;
  const int chunks = hgs_si_chunks(a.H, a.W);
  const float dmin = a.depth_min[b], rng = a.depth_max[b] - dmin + 1e-10f, s = a.depth_global_max[0] + 1e-5f;
  const bool loss = a.grad_loss_sparsity || a.grad_loss_opaque;
  const float gls = a.grad_loss_sparsity ? a.grad_loss_sparsity[0] : 0.0f, glo = a.grad_loss_opaque ? a.grad_loss_opaque[0] : 0.0f;
  const float invN = (float)(1.0 / ((double)a.B * (double)HW));
  const float sy = (float)a.H / (float)a.h, sx = (float)a.W / (float)a.w;
  float s1 = 0.0f, s2 = 0.0f, sg = 0.0f;
  for (int c = p; c < chunks; c += P) {
    float v[4];
    long long first;
    const int cnt = si_chunk_load(plane, HW, c, v, first);
    int y = (int)((uint32_t)first / (uint32_t)a.W), x = (int)((uint32_t)first % (uint32_t)a.W);   // B H W < 2^31
#pragma unroll
    for (int k = 0; k < 4; ++k, ++x) {
      if (k < cnt) {
        const float d = v[k];
        if (x >= a.W) { x -= a.W; ++y; }          // (once is enough: x < W before the step)
        if (a.grad_depth) {
          const float G = si_gather_depth_grad(a, b, y, x, sy, sx);
          s1 += G;
          s2 += G * ((d - dmin) / rng);
        }
        if (loss) {
          const float op = d / s;
          sg += si_dloss_dop(op, gls, glo, invN) * op;
        }
      }
    }
  }
  s1 = si_block_sum(s1, red);
  s2 = si_block_sum(s2, red);
  sg = si_block_sum(sg, red);
  if (threadIdx.x == 0) {
    float* ws = static_cast<float*>(a.workspace);
    const size_t n = (size_t)a.B * P, at = (size_t)b * P + p;
    ws[at] = s1;
    ws[n + at] = s2;
    ws[2 * n + at] = sg;
  }
}

extern "C" __global__ void __launch_bounds__(HGS_SI_THREADS)
hgs_k_si_bwd_finish(const hgs_step_images_args a, const int P) {
  __shared__ double redd[HGS_SI_WAVES];
  float* ws = static_cast<float*>(a.workspace);
  const size_t n = (size_t)a.B * P;
  float* share = ws + HGS_SI_WS_BWD_WORDS * n;
  double sg = 0.0;
  for (int b = 0; b < a.B; ++b) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < P; i += HGS_SI_THREADS) {
      const size_t at = (size_t)b * P + i;
      s1 += (double)ws[at];
      s2 += (double)ws[n + at];
      sg += (double)ws[2 * n + at];
    }
    s1 = si_block_sum(s1, redd);
    s2 = si_block_sum(s2, redd);
    if (threadIdx.x == 0) {
      // nd = (d - dmin) / r, r = dmax - dmin + 1e-10:  dL/dr = -sum(G nd) / r,  dL/ddmax = dL/dr,  dL/ddmin = -sum(G) / r - dL/dr
      const double r = (double)(a.depth_max[b] - a.depth_min[b] + 1e-10f);
      const double dr = -s2 / r, dmin = -s1 / r - dr;
      share[b] = (float)(dmin / (double)a.tie_counts[b]);
      share[a.B + b] = (float)(dr / (double)a.tie_counts[a.B + b]);
    }
  }
  sg = si_block_sum(sg, redd);
  if (threadIdx.x == 0) {
    // op = d / s, s = g + 1e-5:  dL/dg = -sum(dL/dop op) / s
    const double s = (double)(a.depth_global_max[0] + 1e-5f);
    share[2 * a.B] = (float)(-sg / s / (double)a.tie_counts[2 * a.B]);
  }
}

// planes_per_view: 3 colour planes if grad_rgb, + 1 depth plane if want_depth; plane order r, g, b, depth
extern "C" __global__ void __launch_bounds__(HGS_SI_THREADS)
hgs_k_si_bwd_write(const hgs_step_images_args a, const int P, const int blocks_per_plane, const int planes_per_view) {
  const int plane = blockIdx.x / blocks_per_plane, blk = blockIdx.x % blocks_per_plane;
  const int b = plane / planes_per_view;
  const int ch = plane % planes_per_view + (a.grad_rgb ? 0 : 3);
  const bool is_depth = ch == 3;
  const int groups = (a.W + 3) >> 2;
  const long long t = (long long)blk * HGS_SI_THREADS + threadIdx.x;
  if (t >= (long long)groups * a.H) return;
  const int y = (int)(t / groups), x0 = (int)(t % groups) * 4;
  const int cnt = min(4, a.W - x0);
  const size_t HW = (size_t)a.H * a.W, hw = (size_t)a.h * a.w;
  const float sy = (float)a.H / (float)a.h, sx = (float)a.W / (float)a.w;
  const bool vec = (a.W & 3) == 0;
  float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!is_depth) {
    const size_t base = ((size_t)b * 3 + ch) * hw;
    if (a.H == 2 * a.h && a.W == 2 * a.w) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) out[k] = (0.5f * 0.5f) * si_load_grad(a.grad_rgb, base + (size_t)(y >> 1) * a.w + ((x0 + k) >> 1), a.half_images);
    } else {
      const int fy = si_first_candidate(y, a.H, a.h);
      float wy[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) wy[j] = si_weight_t(y, fy + j, a.H, a.h, sy);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          const int x = x0 + k, fx = si_first_candidate(x, a.W, a.w);
          float acc = 0.0f;
          for (int j = 0; j < 5; ++j) {
            if (wy[j] == 0.0f) continue;
            for (int i = 0; i < 5; ++i) {
              const float wx = si_weight_t(x, fx + i, a.W, a.w, sx);
              if (wx == 0.0f) continue;
              acc += (wy[j] * wx) * si_load_grad(a.grad_rgb, base + (size_t)(fy + j) * a.w + (fx + i), a.half_images);
            }
          }
          out[k] = acc;
        }
      }
    }
    float* o = a.grad_render + ((size_t)b * 3 + ch) * HW + (size_t)y * a.W + x0;
    if (vec) {
      *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < cnt) o[k] = out[k];
    }
    return;
  }

  const float* ws = static_cast<const float*>(a.workspace);
  const float* share = ws + HGS_SI_WS_BWD_WORDS * (size_t)a.B * P;
  const float dmin = a.depth_min[b], dmax = a.depth_max[b], g = a.depth_global_max[0];
  const float rng = dmax - dmin + 1e-10f, s = g + 1e-5f;
  const bool loss = a.grad_loss_sparsity || a.grad_loss_opaque;
  const float gls = a.grad_loss_sparsity ? a.grad_loss_sparsity[0] : 0.0f, glo = a.grad_loss_opaque ? a.grad_loss_opaque[0] : 0.0f;
  const float invN = (float)(1.0 / ((double)a.B * (double)HW));
  const float sh_min = share[b], sh_max = share[a.B + b], sh_g = share[2 * a.B];
  const float* __restrict__ drow = a.depth + (size_t)b * HW + (size_t)y * a.W + x0;
  float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (vec) {
    const float4 q = *reinterpret_cast<const float4*>(drow);
    d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) d[k] = drow[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < cnt) {
      float r = 0.0f;
      if (a.grad_depth) r += si_gather_depth_grad(a, b, y, x0 + k, sy, sx) / rng;
      if (loss) r += si_dloss_dop(d[k] / s, gls, glo, invN) / s;
      // amin / amax / max() give every element equal to the extremum an equal share
      if (d[k] == dmin) r += sh_min;
      if (d[k] == dmax) r += sh_max;
      if (d[k] == g) r += sh_g;
      out[k] = r;
    }
  }
  float* o = a.grad_depth_in + (size_t)b * HW + (size_t)y * a.W + x0;
  if (vec) {
    *reinterpret_cast<float4*>(o) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) o[k] = out[k];
  }
}
