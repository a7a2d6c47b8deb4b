// lbs.hip - posing a skinned body (SMPL-X and its kin) on the device: linear blend skinning in two launches
// (include/hgs_rast.h: hgs_lbs_pose states the arithmetic and its order).
//
// Reference code replaced: the per-frame `smplx` forward on the CPU plus the numpy recentring and the upload of
// /root/reference/animation.py:273-330, :552-556.  [UPSTREAM-KNOWLEDGE] the computation is the `smplx` package's lbs().
//
// hgs_k_lbs_joints   one wave per frame, lane j = joint j: Rodrigues, the pose feature pf, the kinematic chain (level by
//                    level through LDS: a round finishes every joint whose parent is finished, so a chain of depth J - 1
//                    takes J - 1 rounds and the SMPL-X tree nine), A_j and the posed joints.
// hgs_k_lbs_skin_*   the hot part: v_posed = v_shaped + pf . posedirs is a sweep over the K x 3V table (61 MB at SMPL-X
//                    size), then the weighted sum of the joint transforms.  A workgroup of 512 threads owns 64 vertices
//                    and a tile of NF frames.  Thread t: vertex group t % 16 (4 vertices = 12 floats = three 16-byte loads
//                    per row, 768 contiguous bytes per row across the 16 lanes), k-slice t / 16 (rows k = slice, slice + 32,
//                    ...: the workgroup reads 32 consecutive rows per step).  Every loaded float serves the NF frames of the
//                    tile from registers; pf sits in LDS as [K][NF], so the NF factors of a row are one or two 16-byte LDS
//                    reads that the 16 lanes of a slice share (broadcast).  The 32 slice sums meet in a fixed tree: two
//                    cross-lane steps inside a wave, then the eight waves in order through LDS.  The last step gives every
//                    (frame, vertex) of the tile a thread, which adds v_shaped, walks the vertex's weight list with A of
//                    the tile in LDS, applies transl and the caller's affine and stores.  No atomics anywhere.
//
// hgs_k_lbs_skin_f1 (NF = 1) serves a call of one frame, hgs_k_lbs_skin_f8 (NF = HGS_LBS_FRAME_TILE) every other call;
// a frame's instruction sequence does not depend on NF, on its place in the tile or on the other frames.
#include "hgs_common.h"

#define HGS_LBS_THREADS 512
#define HGS_LBS_WAVES (HGS_LBS_THREADS / 64)
#define HGS_LBS_LANES 16                                   // lanes of a k-slice (8: 328 workgroups at SMPL-X size instead of
                                                           // 164, and slower - 21 against 18.6 us for one frame, 477 against 286 us for 136)
#define HGS_LBS_SLICES (HGS_LBS_THREADS / HGS_LBS_LANES)   // k-slices of a workgroup
#define HGS_LBS_VERTS (4 * HGS_LBS_LANES)                  // vertices of a workgroup: every lane of a slice owns four
#define HGS_LBS_MAX_K (9 * (HGS_LBS_MAX_JOINTS - 1))

// floats of the workspace in front of each part: A [F][J][12], posed joints [F][J][3], pf [F][9 (J - 1)]
__host__ __device__ __forceinline__ size_t hgs_lbs_ws_joints(int J, int F) { return (size_t)F * J * 12; }
__host__ __device__ __forceinline__ size_t hgs_lbs_ws_pf(int J, int F) { return (size_t)F * J * 15; }

__device__ __forceinline__ float hgs_lbs_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

extern "C" __global__ void __launch_bounds__(64)
hgs_k_lbs_joints(const hgs_lbs_args a) {
  __shared__ float sG[HGS_LBS_MAX_JOINTS][13];     // [R | t] per joint, rows padded to 13 floats (banks)
  const int f = blockIdx.x, j = threadIdx.x, J = a.J;
  const bool on = j < J;
  float* __restrict__ ws = static_cast<float*>(a.workspace);

  float ax = 0.0f, ay = 0.0f, az = 0.0f, jx = 0.0f, jy = 0.0f, jz = 0.0f;
  int par = -1;
  if (on) {
    const float* p = a.poses + ((size_t)f * J + j) * 3;
    ax = p[0]; ay = p[1]; az = p[2];
    jx = a.J_rest[j * 3 + 0]; jy = a.J_rest[j * 3 + 1]; jz = a.J_rest[j * 3 + 2];
    if (j > 0) par = min(max(a.parents[j], 0), J - 1);
  }
  // the offset to the parent, read before the rounds below: a round then waits for LDS only
  float dx = 0.0f, dy = 0.0f, dz = 0.0f;
  if (on && j > 0) { dx = jx - a.J_rest[par * 3 + 0]; dy = jy - a.J_rest[par * 3 + 1]; dz = jz - a.J_rest[par * 3 + 2]; }
  // batch_rodrigues of the package: the 1e-8 enters the angle only
  const float bx = ax + 1e-8f, by = ay + 1e-8f, bz = az + 1e-8f;
  const float angle = sqrtf((bx * bx + by * by) + bz * bz);
  const float kx = ax / angle, ky = ay / angle, kz = az / angle;
  float s, c;
  sincosf(angle, &s, &c);
  const float oc = 1.0f - c;
  float R[9];
  R[0] = 1.0f + oc * (-(kz * kz) - ky * ky);
  R[1] = s * -kz + oc * (ky * kx);
  R[2] = s * ky + oc * (kz * kx);
  R[3] = s * kz + oc * (kx * ky);
  R[4] = 1.0f + oc * (-(kz * kz) - kx * kx);
  R[5] = s * -kx + oc * (kz * ky);
  R[6] = s * -ky + oc * (kx * kz);
  R[7] = s * kx + oc * (ky * kz);
  R[8] = 1.0f + oc * (-(ky * ky) - kx * kx);

  if (on && j > 0 && a.K > 0) {
    float* pf = ws + hgs_lbs_ws_pf(J, a.F) + (size_t)f * a.K + (size_t)(j - 1) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) pf[i] = R[i] - ((i & 3) == 0 ? 1.0f : 0.0f);
  }

  // the chain: G of the root, and of a joint that a broken parents table never reaches, is the local [R | J]
  float G[12] = {R[0], R[1], R[2], jx, R[3], R[4], R[5], jy, R[6], R[7], R[8], jz};
  unsigned long long done = 1ull;
  if (j == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) sG[0][i] = G[i];
  }
  for (int round = 1; round < J; ++round) {
    __syncthreads();
    const bool ready = on && j > 0 && !((done >> j) & 1ull) && ((done >> par) & 1ull);
    if (ready) {
      float P[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) P[i] = sG[par][i];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) G[r * 4 + c] = hgs_lbs_dot3(P[r * 4], P[r * 4 + 1], P[r * 4 + 2], R[c], R[3 + c], R[6 + c]);
        G[r * 4 + 3] = hgs_lbs_dot3(P[r * 4], P[r * 4 + 1], P[r * 4 + 2], dx, dy, dz) + P[r * 4 + 3];
      }
#pragma unroll
      for (int i = 0; i < 12; ++i) sG[j][i] = G[i];
    }
    const unsigned long long now = done | __ballot(ready);
    if (now == done) break;                        // (uniform) every reachable joint is finished
    done = now;
  }

  if (!on) return;
  float* A = ws + ((size_t)f * J + j) * 12;
  float4* A4 = reinterpret_cast<float4*>(A);
  const float tx = G[3] - hgs_lbs_dot3(G[0], G[1], G[2], jx, jy, jz);
  const float ty = G[7] - hgs_lbs_dot3(G[4], G[5], G[6], jx, jy, jz);
  const float tz = G[11] - hgs_lbs_dot3(G[8], G[9], G[10], jx, jy, jz);
  A4[0] = make_float4(G[0], G[1], G[2], tx);
  A4[1] = make_float4(G[4], G[5], G[6], ty);
  A4[2] = make_float4(G[8], G[9], G[10], tz);
  float* pj = ws + hgs_lbs_ws_joints(J, a.F) + ((size_t)f * J + j) * 3;
  pj[0] = G[3]; pj[1] = G[7]; pj[2] = G[11];
  if (a.joints) {
    float ox = G[3], oy = G[7], oz = G[11];
    if (a.transl) { ox = ox + a.transl[f * 3 + 0]; oy = oy + a.transl[f * 3 + 1]; oz = oz + a.transl[f * 3 + 2]; }
    float* o = a.joints + ((size_t)f * J + j) * 3;
    o[0] = (ox - a.centre[0]) * a.scale;
    o[1] = (oy - a.centre[1]) * a.scale;
    o[2] = (oz - a.centre[2]) * a.scale;
  }
}

template <int NF>
__device__ __forceinline__ void hgs_lbs_skin(const hgs_lbs_args& a) {
  __shared__ __attribute__((aligned(16))) float sPf[HGS_LBS_MAX_K * NF];                    // [K][NF]
  __shared__ __attribute__((aligned(16))) float sA[NF * HGS_LBS_MAX_JOINTS * 12];           // [NF][J][12]
  __shared__ float sPart[HGS_LBS_WAVES * NF * HGS_LBS_VERTS * 3];                           // [wave][NF][vertex x 3]
  static_assert(NF * HGS_LBS_VERTS <= HGS_LBS_THREADS, "the last step gives every (frame, vertex) of the tile a thread");
  const int tid = threadIdx.x, V = a.V, J = a.J, K = a.K;
  const uint32_t nvb = (uint32_t)((V + HGS_LBS_VERTS - 1) / HGS_LBS_VERTS);
  const int tile = (int)(blockIdx.x / nvb), vb = (int)(blockIdx.x % nvb);
  const int f0 = tile * NF, nf = min(NF, a.F - f0);
  const float* __restrict__ ws = static_cast<const float*>(a.workspace);

  // stage the tile's pose features ([K][NF], zeros for the frames the tile does not have) and transforms
  {
    const float* __restrict__ pf = ws + hgs_lbs_ws_pf(J, a.F) + (size_t)f0 * K;
    for (int i = tid; i < K * NF; i += HGS_LBS_THREADS) {
      const int f = i / K, k = i - f * K;
      sPf[k * NF + f] = f < nf ? pf[i] : 0.0f;
    }
    const float4* __restrict__ A4 = reinterpret_cast<const float4*>(ws + (size_t)f0 * J * 12);
    float4* sA4 = reinterpret_cast<float4*>(sA);
    for (int i = tid; i < nf * J * 3; i += HGS_LBS_THREADS) sA4[i] = A4[i];
  }
  __syncthreads();

  // the sweep: this thread's 12 columns of the rows of its slice, for the NF frames of the tile
  const int vg = tid & (HGS_LBS_LANES - 1), slice = tid / HGS_LBS_LANES;
  const int v0 = vb * HGS_LBS_VERTS + 4 * vg;
  float acc[NF][12];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int c = 0; c < 12; ++c) acc[f][c] = 0.0f;
  if (v0 < V) {
    const float* __restrict__ pd = a.posedirs + (size_t)3 * v0;
    const size_t stride = (size_t)a.posedirs_stride;
#pragma unroll 2
    for (int k = slice; k < K; k += HGS_LBS_SLICES) {
      const float4* __restrict__ row = reinterpret_cast<const float4*>(pd + (size_t)k * stride);
      const float4 q0 = row[0], q1 = row[1], q2 = row[2];
      const float q[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
      float w[NF];
      if constexpr (NF % 4 == 0) {
#pragma unroll
        for (int g = 0; g < NF / 4; ++g) {
          const float4 w4 = reinterpret_cast<const float4*>(sPf + k * NF)[g];
          w[4 * g] = w4.x; w[4 * g + 1] = w4.y; w[4 * g + 2] = w4.z; w[4 * g + 3] = w4.w;
        }
      } else {
#pragma unroll
        for (int f = 0; f < NF; ++f) w[f] = sPf[k * NF + f];
      }
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[f][c] = acc[f][c] + w[f] * q[c];
    }
  }

  // the 32 slice sums in a fixed tree: (s0 + s1) + (s2 + s3) over the four slices of a wave, then the eight waves in order
  const int wave = tid >> 6;
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      float x = acc[f][c];
#pragma unroll
      for (int m = HGS_LBS_LANES; m < 64; m <<= 1) x = x + __shfl_xor(x, m);
      if ((tid & 63) < HGS_LBS_LANES) sPart[(wave * NF + f) * (HGS_LBS_VERTS * 3) + vg * 12 + c] = x;
    }
  __syncthreads();

  const int v = tid % HGS_LBS_VERTS, f = tid / HGS_LBS_VERTS, gv = vb * HGS_LBS_VERTS + v;
  if (f >= nf || gv >= V) return;
  float p[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float sum = sPart[f * (HGS_LBS_VERTS * 3) + v * 3 + c];
#pragma unroll
    for (int w = 1; w < HGS_LBS_WAVES; ++w) sum = sum + sPart[(w * NF + f) * (HGS_LBS_VERTS * 3) + v * 3 + c];
    p[c] = a.v_shaped[(size_t)gv * 3 + c] + sum;
  }
  float ox = 0.0f, oy = 0.0f, oz = 0.0f;
  const int W = a.weight_width;
  const int32_t* __restrict__ wj = a.weight_joint + (size_t)gv * W;
  const float* __restrict__ wv = a.weight_value + (size_t)gv * W;
  const float4* sA4 = reinterpret_cast<const float4*>(sA) + (size_t)f * J * 3;
  for (int i = 0; i < W; ++i) {
    const int jt = min(max(wj[i], 0), J - 1);
    const float wt = wv[i];
    const float4 r0 = sA4[jt * 3], r1 = sA4[jt * 3 + 1], r2 = sA4[jt * 3 + 2];
    ox = ox + wt * (hgs_lbs_dot3(r0.x, r0.y, r0.z, p[0], p[1], p[2]) + r0.w);
    oy = oy + wt * (hgs_lbs_dot3(r1.x, r1.y, r1.z, p[0], p[1], p[2]) + r1.w);
    oz = oz + wt * (hgs_lbs_dot3(r2.x, r2.y, r2.z, p[0], p[1], p[2]) + r2.w);
  }
  const int fr = f0 + f;
  if (a.transl) { ox = ox + a.transl[fr * 3 + 0]; oy = oy + a.transl[fr * 3 + 1]; oz = oz + a.transl[fr * 3 + 2]; }
  float* o = a.vertices + ((size_t)fr * V + gv) * 3;
  o[0] = (ox - a.centre[0]) * a.scale;
  o[1] = (oy - a.centre[1]) * a.scale;
  o[2] = (oz - a.centre[2]) * a.scale;
}

extern "C" __global__ void __launch_bounds__(HGS_LBS_THREADS)
hgs_k_lbs_skin_f1(const hgs_lbs_args a) { hgs_lbs_skin<1>(a); }

extern "C" __global__ void __launch_bounds__(HGS_LBS_THREADS)
hgs_k_lbs_skin_f8(const hgs_lbs_args a) { hgs_lbs_skin<HGS_LBS_FRAME_TILE>(a); }
