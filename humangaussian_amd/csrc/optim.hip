// optim.hip - the optimizer step of the Gaussian model as ONE HIP launch over all parameter tensors
// (include/hgs_rast.h: hgs_adam_step).  HBM-bound elementwise work: per element three 4-byte reads of state, one of
// the gradient and three writes; no atomics, no LDS, no scratch.
//
// Reference code replaced: torch.optim.Adam over six groups of one tensor each
// (gaussiansplatting/scene/gaussian_model.py:156-165) - a chain of elementwise torch kernels per group, every step.
//
// Launch shape: the argument struct travels BY VALUE (kernel arguments: no device-side table, no H2D copy).  Tensor k
// owns the workgroups [block_start[k], block_start[k + 1]); a workgroup finds its tensor by walking that prefix (uniform:
// scalar loads) and grid-strides over the tensor's elements with its siblings.  A tensor whose four pointers are 16-byte
// aligned moves as float4 (its last n mod 4 elements one by one, in its first workgroup); any other tensor moves element
// by element.  The arithmetic per element is the same in both forms, in the order the header states (-ffp-contract=off).
#include "hgs_common.h"

#define HGS_ADAM_THREADS 256
#define HGS_ADAM_BLOCK_ELEMS 1024          // elements a workgroup takes per grid stride (one float4 per thread)
#define HGS_ADAM_MAX_BLOCKS 2048           // 256 CUs x 8 workgroups: the cap for a streaming kernel; the rest is grid-strided

struct AdamScalars { float step_size, bc2_sqrt, w1, beta2, w2, eps; };

__device__ __forceinline__ void hgs_adam_elem(const AdamScalars& s, float g, float& p, float& m, float& v) {
  m = m + (g - m) * s.w1;
  v = v * s.beta2 + (g * g) * s.w2;
  const float d = sqrtf(v) / s.bc2_sqrt + s.eps;
  p = p - s.step_size * (m / d);
}

// row of element e of a tensor of n elements in rows of rf floats (32-bit division where the tensor allows it)
__device__ __forceinline__ long long hgs_adam_row(long long e, long long n, int rf) {
  return n <= 0xffffffffll ? (long long)((uint32_t)e / (uint32_t)rf) : e / rf;
}

extern "C" __global__ void __launch_bounds__(HGS_ADAM_THREADS)
hgs_k_adam(const hgs_adam_args a) {
  int k = 0;
  while (k + 1 < a.num_tensors && blockIdx.x >= a.block_start[k + 1]) ++k;
  const hgs_adam_tensor& t = a.t[k];
  const long long nb = (long long)(a.block_start[k + 1] - a.block_start[k]);
  const long long lb = (long long)(blockIdx.x - a.block_start[k]);
  const long long n = (long long)t.rows * t.row_floats;
  const AdamScalars s = {t.step_size, t.bc2_sqrt, t.w1, t.beta2, t.w2, t.eps};
  float* __restrict__ P = t.param;
  const float* __restrict__ G = t.grad;
  float* __restrict__ M = t.exp_avg;
  float* __restrict__ V = t.exp_avg_sq;
  const uint8_t* __restrict__ vis = a.visible;
  const int rf = t.row_floats;
  const bool vec = (((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V) & 15) == 0;
  const long long n_vec = vec ? (n & ~3ll) : 0;      // elements [0, n_vec) move as float4, [n_vec, n) one by one

  for (long long e = (lb * HGS_ADAM_THREADS + threadIdx.x) * 4; e < n_vec; e += nb * HGS_ADAM_BLOCK_ELEMS) {
    bool on[4] = {true, true, true, true};
    if (vis) {
      for (int c = 0; c < 4; ++c) on[c] = vis[hgs_adam_row(e + c, n, rf)] != 0;
      if (!(on[0] || on[1] || on[2] || on[3])) continue;
    }
    const float4 g4 = *reinterpret_cast<const float4*>(G + e);
    float4 p4 = *reinterpret_cast<const float4*>(P + e);
    float4 m4 = *reinterpret_cast<const float4*>(M + e);
    float4 v4 = *reinterpret_cast<const float4*>(V + e);
    const float4 p0 = p4, m0 = m4, v0 = v4;
    hgs_adam_elem(s, g4.x, p4.x, m4.x, v4.x);
    hgs_adam_elem(s, g4.y, p4.y, m4.y, v4.y);
    hgs_adam_elem(s, g4.z, p4.z, m4.z, v4.z);
    hgs_adam_elem(s, g4.w, p4.w, m4.w, v4.w);
    if (vis) {                                       // a row that is not visible keeps its bits
      if (!on[0]) { p4.x = p0.x; m4.x = m0.x; v4.x = v0.x; }
      if (!on[1]) { p4.y = p0.y; m4.y = m0.y; v4.y = v0.y; }
      if (!on[2]) { p4.z = p0.z; m4.z = m0.z; v4.z = v0.z; }
      if (!on[3]) { p4.w = p0.w; m4.w = m0.w; v4.w = v0.w; }
    }
    *reinterpret_cast<float4*>(P + e) = p4;
    *reinterpret_cast<float4*>(M + e) = m4;
    *reinterpret_cast<float4*>(V + e) = v4;
  }

  // scalar form: the tail of an aligned tensor (fewer than four elements: the tensor's first workgroup takes them), or
  // the whole of a tensor that is not aligned
  const long long stride = vec ? HGS_ADAM_THREADS : nb * HGS_ADAM_THREADS;
  if (vec && lb != 0) return;
  for (long long e = n_vec + lb * HGS_ADAM_THREADS + threadIdx.x; e < n; e += stride) {
    if (vis && !vis[hgs_adam_row(e, n, rf)]) continue;
    float p = P[e], m = M[e], v = V[e];
    hgs_adam_elem(s, G[e], p, m, v);
    P[e] = p;
    M[e] = m;
    V[e] = v;
  }
}
