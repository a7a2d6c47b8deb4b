// photometric.hip - the photometric loss of image fitting: L1 + D-SSIM forward and backward and the sums PSNR needs, two
// launches forward and one backward (include/hgs_rast.h: hgs_photometric_* states the formulas).
//
// Reference code replaced: gaussiansplatting/utils/loss_utils.py (l1_loss, ssim / _ssim: five depthwise 11 x 11 conv2d and
// about fifteen elementwise kernels forward, their autograd chain backward) and utils/image_utils.py (psnr).
//
// One workgroup of 256 threads owns one tile of HGS_PM_TILE_H x HGS_PM_TILE_W pixels of one (b, c) plane:
//   load        the tile and its halo of 5 (42 x 42) of x and y into LDS, zero outside the plane (conv2d's padding)
//   rows        a thread takes 4 neighbouring columns of one halo row: 14 x and 14 y from LDS, the 11 taps of the five
//               quantities x, y, x x, y y, x y -> hb[5][42][32]
//   columns     a thread takes 4 neighbouring rows of one column: 14 values per quantity from hb -> mu1, mu2, E[xx], E[yy],
//               E[xy] of its 4 pixels; the SSIM map value, the three derivative maps (with_grad), |x - y|, (x - y)^2
//   sums        the thread's 4 pixels in order, a fixed tree over the lanes, the four waves in order: one partial per sum
// LDS row strides 43 and 33 words: every wave access of the two passes falls on distinct banks.  42 KB of LDS: three
// workgroups per CU.  The backward is the same tile and the same two passes over the three derivative maps (38 KB).
//
// hgs_k_pm_forward   F1  per tile: the derivative maps and three partials
// hgs_k_pm_finish    F2  one workgroup of 16 waves: a wave per plane adds its partials in fp64; then the per-image and the
//                        overall means, loss, psnr
// hgs_k_pm_backward  B1  per tile: grad_image
#include "hgs_common.h"

#define HGS_PM_THREADS 256
#define HGS_PM_FINISH_THREADS 1024
#define PM_HALO 5
#define PM_TAPS 11
#define PM_LH (HGS_PM_TILE_H + 2 * PM_HALO)
#define PM_LW (HGS_PM_TILE_W + 2 * PM_HALO)
#define PM_IN_STRIDE (PM_LW + 1)
#define PM_HB_STRIDE (HGS_PM_TILE_W + 1)
#define PM_ROW_ITEMS (PM_LH * (HGS_PM_TILE_W / 4))
#define PM_SPAN (4 + PM_TAPS - 1)      // inputs of 4 neighbouring outputs of one pass
static_assert(HGS_PM_TILE_W == 32 && HGS_PM_TILE_H * HGS_PM_TILE_W == 4 * HGS_PM_THREADS,
              "the column pass gives a thread 4 rows of one of 32 columns");
static_assert(HGS_PM_FINISH_CHUNK == 64, "a wave adds a plane's partials");

// words of the workspace: [3][planes][tiles] fp32 partials (ssim, |d|, d^2), [3][planes] fp64 plane sums, then (with_grad)
// [3][N] fp32 derivative maps (dS/dmu1, dS/ds1, dS/ds12); api.hip carves it
struct PmCarve { size_t partials, plane_sums, maps, total; };
__host__ __device__ __forceinline__ int pm_tiles_x(int W) { return (W + HGS_PM_TILE_W - 1) / HGS_PM_TILE_W; }
__host__ __device__ __forceinline__ int pm_tiles(int H, int W) {
  return pm_tiles_x(W) * ((H + HGS_PM_TILE_H - 1) / HGS_PM_TILE_H);
}
__host__ __device__ __forceinline__ PmCarve pm_carve(int B, int C, int H, int W, int with_grad) {
  const size_t planes = (size_t)B * C;
  PmCarve c;
  c.partials = 0;
  c.plane_sums = (3 * planes * pm_tiles(H, W) * 4 + 255) / 256 * 256;
  c.maps = (c.plane_sums + 3 * planes * 8 + 255) / 256 * 256;
  c.total = with_grad ? (c.maps + 3 * planes * H * W * 4 + 255) / 256 * 256 : c.maps;
  return c;
}

// fixed order: lanes by halving strides, then the four waves in order
__device__ __forceinline__ float pm_block_sum(float v, float* lds) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// the 11 taps over v[j .. j + 10], added in ascending order from 0
__device__ __forceinline__ float pm_taps(const float* v, int j) {
  constexpr float w[PM_TAPS] = HGS_PM_WINDOW;
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < PM_TAPS; ++k) acc += w[k] * v[j + k];
  return acc;
}

// the tile plus halo of one plane into LDS, zero outside the plane
__device__ __forceinline__ void pm_load_halo(const float* __restrict__ plane, int H, int W, int y0, int x0, float* lds) {
  for (int i = threadIdx.x; i < PM_LH * PM_LW; i += HGS_PM_THREADS) {
    const int r = i / PM_LW, c = i - r * PM_LW;
    const int gy = y0 + r - PM_HALO, gx = x0 + c - PM_HALO;
    float v = 0.0f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = plane[(size_t)gy * W + gx];
    lds[r * PM_IN_STRIDE + c] = v;
  }
}

// the column pass of one quantity for the thread's 4 rows r0 .. r0 + 3 of column c
__device__ __forceinline__ void pm_columns(const float* hq, int r0, int c, float out[4]) {
  float v[PM_SPAN];
#pragma unroll
  for (int k = 0; k < PM_SPAN; ++k) v[k] = hq[(r0 + k) * PM_HB_STRIDE + c];
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = pm_taps(v, j);
}

extern "C" __global__ void __launch_bounds__(HGS_PM_THREADS)
hgs_k_pm_forward(const hgs_photometric_args a, const int tiles_x) {
  __shared__ float sx[PM_LH * PM_IN_STRIDE], sy[PM_LH * PM_IN_STRIDE];
  __shared__ float hb[5][PM_LH * PM_HB_STRIDE];
  __shared__ float red[3][4];
  const int plane = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x, planes = gridDim.y;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * HGS_PM_TILE_H, x0 = tx * HGS_PM_TILE_W;
  const size_t HW = (size_t)a.H * a.W, base = (size_t)plane * HW;
  pm_load_halo(a.image + base, a.H, a.W, y0, x0, sx);
  pm_load_halo(a.gt + base, a.H, a.W, y0, x0, sy);
  __syncthreads();
  for (int it = threadIdx.x; it < PM_ROW_ITEMS; it += HGS_PM_THREADS) {
    const int r = it / (HGS_PM_TILE_W / 4), c0 = (it - r * (HGS_PM_TILE_W / 4)) * 4;
    float vx[PM_SPAN], vy[PM_SPAN], vxx[PM_SPAN], vyy[PM_SPAN], vxy[PM_SPAN];
#pragma unroll
    for (int k = 0; k < PM_SPAN; ++k) {
      vx[k] = sx[r * PM_IN_STRIDE + c0 + k];
      vy[k] = sy[r * PM_IN_STRIDE + c0 + k];
      vxx[k] = vx[k] * vx[k];
      vyy[k] = vy[k] * vy[k];
      vxy[k] = vx[k] * vy[k];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = r * PM_HB_STRIDE + c0 + j;
      hb[0][o] = pm_taps(vx, j);
      hb[1][o] = pm_taps(vy, j);
      hb[2][o] = pm_taps(vxx, j);
      hb[3][o] = pm_taps(vyy, j);
      hb[4][o] = pm_taps(vxy, j);
    }
  }
  __syncthreads();
  const int c = threadIdx.x & (HGS_PM_TILE_W - 1), r0 = (threadIdx.x / HGS_PM_TILE_W) * 4;
  float mu1[4], mu2[4], e11[4], e22[4], e12[4];
  pm_columns(hb[0], r0, c, mu1);
  pm_columns(hb[1], r0, c, mu2);
  pm_columns(hb[2], r0, c, e11);
  pm_columns(hb[3], r0, c, e22);
  pm_columns(hb[4], r0, c, e12);
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  float* __restrict__ maps = reinterpret_cast<float*>(static_cast<char*>(a.workspace) + pm_carve(a.B, a.C, a.H, a.W, 1).maps);
  const size_t N = (size_t)planes * HW;
  float sum_s = 0.0f, sum_a = 0.0f, sum_q = 0.0f;
  const int gx = x0 + c;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = y0 + r0 + j;
    if (gy < a.H && gx < a.W) {
      const float m1 = mu1[j], m2 = mu2[j];
      const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
      const float s1 = e11[j] - m11, s2 = e22[j] - m22, s12 = e12[j] - m12;
      const float A1 = 2.0f * m12 + C1, A2 = 2.0f * s12 + C2, B1 = m11 + m22 + C1, B2 = s1 + s2 + C2;
      const float den = B1 * B2;
      const float S = (A1 * A2) / den;
      const float x = sx[(r0 + j + PM_HALO) * PM_IN_STRIDE + c + PM_HALO], y = sy[(r0 + j + PM_HALO) * PM_IN_STRIDE + c + PM_HALO];
      const float d = x - y;
      sum_s += S;
      sum_a += fabsf(d);
      sum_q += d * d;
      if (a.with_grad) {
        const size_t p = base + (size_t)gy * a.W + gx;
        maps[p] = 2.0f * (m2 * (A2 - A1) + m1 * S * (B1 - B2)) / den;
        maps[N + p] = -S / B2;
        maps[2 * N + p] = 2.0f * A1 / den;
      }
    }
  }
  sum_s = pm_block_sum(sum_s, red[0]);
  sum_a = pm_block_sum(sum_a, red[1]);
  sum_q = pm_block_sum(sum_q, red[2]);
  if (threadIdx.x == 0) {
    float* __restrict__ part = static_cast<float*>(a.workspace);
    const size_t n = (size_t)planes * tiles, i = (size_t)plane * tiles + tile;
    part[i] = sum_s;
    part[n + i] = sum_a;
    part[2 * n + i] = sum_q;
  }
}

__device__ __forceinline__ float pm_psnr(double mse) {
  const float m = (float)mse;                                   // the reference's mse is an fp32 mean
  return (float)(20.0 * log10(1.0 / sqrt((double)m)));
}

// One workgroup.  Wave v adds the partials of planes v, v + 16, ...; then threads add planes.
extern "C" __global__ void __launch_bounds__(HGS_PM_FINISH_THREADS)
hgs_k_pm_finish(const hgs_photometric_args a, const int tiles) {
  __shared__ double red[2][HGS_PM_FINISH_THREADS / 64];
  const int planes = a.B * a.C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const PmCarve cv = pm_carve(a.B, a.C, a.H, a.W, 0);
  const float* __restrict__ part = static_cast<const float*>(a.workspace);
  double* psum = reinterpret_cast<double*>(static_cast<char*>(a.workspace) + cv.plane_sums);
  const size_t n = (size_t)planes * tiles;
  for (int plane = wave; plane < planes; plane += HGS_PM_FINISH_THREADS / 64) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = lane; i < tiles; i += HGS_PM_FINISH_CHUNK) {
      const size_t o = (size_t)plane * tiles + i;
      s[0] += (double)part[o];
      s[1] += (double)part[n + o];
      s[2] += (double)part[2 * n + o];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int st = 32; st > 0; st >>= 1) s[q] += __shfl_down(s[q], st, 64);
    }
    if (lane == 0) {
      psum[plane] = s[0];
      psum[planes + plane] = s[1];
      psum[2 * planes + plane] = s[2];
      a.sqerr[plane] = (float)s[2];
    }
  }
  __syncthreads();                      // the plane sums, written by this workgroup, are visible to all of it
  const double HW = (double)a.H * (double)a.W, CHW = HW * (double)a.C;
  for (int b = threadIdx.x; b < a.B; b += HGS_PM_FINISH_THREADS) {
    double s = 0.0, q = 0.0;
    for (int c = 0; c < a.C; ++c) {
      s += psum[b * a.C + c];
      q += psum[2 * planes + b * a.C + c];
    }
    a.ssim_image[b] = (float)(s / CHW);
    if (!a.psnr_per_plane) a.psnr[b] = pm_psnr(q / CHW);
  }
  if (a.psnr_per_plane)
    for (int p = threadIdx.x; p < planes; p += HGS_PM_FINISH_THREADS) a.psnr[p] = pm_psnr(psum[2 * planes + p] / HW);
  double t0 = 0.0, t1 = 0.0;
  for (int p = threadIdx.x; p < planes; p += HGS_PM_FINISH_THREADS) {
    t0 += psum[p];
    t1 += psum[planes + p];
  }
#pragma unroll
  for (int st = 32; st > 0; st >>= 1) {
    t0 += __shfl_down(t0, st, 64);
    t1 += __shfl_down(t1, st, 64);
  }
  if (lane == 0) { red[0][wave] = t0; red[1][wave] = t1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double u0 = 0.0, u1 = 0.0;
    for (int v = 0; v < HGS_PM_FINISH_THREADS / 64; ++v) { u0 += red[0][v]; u1 += red[1][v]; }
    const double N = CHW * (double)a.B;
    const float ssim = (float)(u0 / N), l1 = (float)(u1 / N);
    *a.ssim = ssim;
    *a.l1 = l1;
    *a.loss = a.weight_l1 * l1 + a.weight_dssim * (1.0f - ssim);
  }
}

extern "C" __global__ void __launch_bounds__(HGS_PM_THREADS)
hgs_k_pm_backward(const hgs_photometric_args a, const int tiles_x) {
  __shared__ float sm[3][PM_LH * PM_IN_STRIDE];
  __shared__ float hb[3][PM_LH * PM_HB_STRIDE];
  const int plane = blockIdx.y, tile = blockIdx.x, planes = gridDim.y;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * HGS_PM_TILE_H, x0 = tx * HGS_PM_TILE_W;
  const size_t HW = (size_t)a.H * a.W, base = (size_t)plane * HW, N = (size_t)planes * HW;
  const int b = plane / a.C;
  const float g_loss = a.grad_loss ? *a.grad_loss : 0.0f;
  const float g_mean = (a.grad_ssim ? *a.grad_ssim : 0.0f) - a.weight_dssim * g_loss;
  const float gs = (g_mean / (float)a.B + (a.grad_ssim_image ? a.grad_ssim_image[b] : 0.0f)) / (float)((size_t)a.C * HW);
  const float gl = ((a.grad_l1 ? *a.grad_l1 : 0.0f) + a.weight_l1 * g_loss) / (float)N;
  const int c = threadIdx.x & (HGS_PM_TILE_W - 1), r0 = (threadIdx.x / HGS_PM_TILE_W) * 4;
  float f[3][4] = {};
  if (gs != 0.0f) {                     // the same for the whole workgroup: b is
    const float* __restrict__ maps = reinterpret_cast<const float*>(static_cast<const char*>(a.workspace) + pm_carve(a.B, a.C, a.H, a.W, 1).maps);
#pragma unroll
    for (int q = 0; q < 3; ++q) pm_load_halo(maps + q * N + base, a.H, a.W, y0, x0, sm[q]);
    __syncthreads();
    for (int it = threadIdx.x; it < PM_ROW_ITEMS; it += HGS_PM_THREADS) {
      const int r = it / (HGS_PM_TILE_W / 4), c0 = (it - r * (HGS_PM_TILE_W / 4)) * 4;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        float v[PM_SPAN];
#pragma unroll
        for (int k = 0; k < PM_SPAN; ++k) v[k] = sm[q][r * PM_IN_STRIDE + c0 + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) hb[q][r * PM_HB_STRIDE + c0 + j] = pm_taps(v, j);
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) pm_columns(hb[q], r0, c, f[q]);
  }
  const int gx = x0 + c;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = y0 + r0 + j;
    if (gy < a.H && gx < a.W) {
      const size_t p = base + (size_t)gy * a.W + gx;
      const float x = a.image[p], y = a.gt[p], d = x - y;
      const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
      const float t = f[0][j] + (2.0f * x) * f[1][j] + y * f[2][j];
      a.grad_image[p] = gs * t + gl * sg;
    }
  }
}
