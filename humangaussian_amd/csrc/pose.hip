// pose.hip - the pose-control images of a training step: B views of one skeleton in one launch
// (include/hgs_rast.h: hgs_pose_draw states the projection, the records and the coverage rules).
//
// Reference code replaced: per view a device-to-host copy of the mvp matrix, a cv2 drawing on the CPU and the upload of
// the float image (the reference's threestudio/systems/GaussianDreamer.py:268-287, threestudio/utils/poser.py:361-459).
//
// hgs_k_pose_draw   grid (tiles, B), 256 threads, one 64 x 16 pixel tile of one view per workgroup.
//   phase A  every workgroup recomputes its view's K <= 18 projections, the occlusion rules and the R <= 35 records in
//            LDS (a few hundred flops: cheaper than a second launch or a hand-off between workgroups); the workgroup of
//            tile 0 writes kp and records out.
//   cull     the first wave tests every record's bounding box against the tile and compacts the survivors, in order,
//            with one ballot.  Most tiles of a skeleton image have none and only write zeros.
//   raster   a thread owns 4 consecutive pixels of a row (48 contiguous bytes of fp32 output: three 16-byte stores; a
//            scalar tail where the row is not 16-byte aligned or the four pixels do not all exist) and walks the
//            survivors in order.  Differences, dot and cross products fit int32 (hgs_rast.h derives the bounds); only the
//            squares are taken in int64.
// The shape (tile, 4 pixels per thread, recomputing phase A everywhere) is a judgement, not a measured optimum.
#include "hgs_common.h"
#define HGS_POSE_TRIG_QUAL __constant__ static const
#include "pose_trig.h"

#define HGS_POSE_THREADS 256
#define HGS_POSE_TILE_W 64
#define HGS_POSE_TILE_H 16
#define HGS_POSE_MAX_K 18
#define HGS_POSE_MAX_RECORDS (HGS_POSE_MAX_COLOURS + HGS_POSE_MAX_LIMBS)
#define HGS_POSE_COORD_MAX 8191.0f
#define HGS_POSE_REC_CAPSULE 1
#define HGS_POSE_REC_DISC 2
#define HGS_POSE_REC_ELLIPSE 3

__host__ __device__ __forceinline__ int hgs_pose_num_records(int style) {
  return style == HGS_POSE_HUMANSD ? HGS_POSE_MAX_LIMBS - 1 : HGS_POSE_MAX_RECORDS;
}

// is the pixel (px, py) inside the record?  (the rules of hgs_rast.h, exactly)
__device__ __forceinline__ bool hgs_pose_covers(const int* __restrict__ r, int px, int py) {
  const int type = r[0];
  if (type == HGS_POSE_REC_CAPSULE) {
    const int apx = px - r[1], apy = py - r[2], abx = r[3] - r[1], aby = r[4] - r[2];
    const int t = apx * abx + apy * aby, L = abx * abx + aby * aby;
    const long long w2 = (long long)r[5] * r[5];
    if (t <= 0) return 4ll * (apx * apx + apy * apy) <= w2;
    if (t >= L) {
      const int bpx = px - r[3], bpy = py - r[4];
      return 4ll * (bpx * bpx + bpy * bpy) <= w2;
    }
    const long long cr = (long long)(apx * aby - apy * abx);
    return 4ll * cr * cr <= w2 * L;
  }
  const int dx = px - r[1], dy = py - r[2];
  if (type == HGS_POSE_REC_DISC) return dx * dx + dy * dy <= r[3];
  // the ellipse; r[6] and r[7] of the LDS copy hold C and S (the global record has 0 and rgb there)
  const int a = r[3], b = r[5], C = r[6], S = r[7];
  const int u = dx * C + dy * S, v = dy * C - dx * S;
  if (abs(u) > a * HGS_POSE_TRIG_ONE || abs(v) > b * HGS_POSE_TRIG_ONE) return false;
  const long long a2 = (long long)a * a, b2 = (long long)b * b;
  return (long long)u * u * b2 + (long long)v * v * a2 <= a2 * b2 * ((long long)HGS_POSE_TRIG_ONE * HGS_POSE_TRIG_ONE);
}

extern "C" __global__ void __launch_bounds__(HGS_POSE_THREADS)
hgs_k_pose_draw(const hgs_pose_args a) {
  __shared__ float sX[HGS_POSE_MAX_K], sY[HGS_POSE_MAX_K], sZ[HGS_POSE_MAX_K], sConf[HGS_POSE_MAX_K];
  __shared__ int sUse[HGS_POSE_MAX_K];
  __shared__ int sSumPos;
  __shared__ int sRec[HGS_POSE_MAX_RECORDS][HGS_POSE_RECORD_INTS];   // the records; an ellipse keeps C, S in [6], [7]
  __shared__ int sRgb[HGS_POSE_MAX_RECORDS];
  __shared__ int sList[HGS_POSE_MAX_RECORDS];
  __shared__ int sCount;
  const int tid = threadIdx.x, view = blockIdx.y, K = a.K, H = a.H, W = a.W;
  const bool humansd = a.style == HGS_POSE_HUMANSD;
  const int R = hgs_pose_num_records(a.style);

  // ---- phase A: projection
  if (tid < K) {
    const float* __restrict__ m = a.mvp + (size_t)view * 16;
    const float* __restrict__ p = a.points + tid * 4;
    float clip[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      clip[c] = __fmaf_rn(m[c * 4 + 3], p[3], __fmaf_rn(m[c * 4 + 2], p[2], __fmaf_rn(m[c * 4 + 1], p[1], m[c * 4] * p[0])));
    const float nx = __fdiv_rn(clip[0], clip[3]), ny = __fdiv_rn(clip[1], clip[3]), nz = __fdiv_rn(clip[2], clip[3]);
    const float xs = (nx + 1.0f) * 0.5f * (float)H, ys = (ny + 1.0f) * 0.5f * (float)W;
    sX[tid] = xs; sY[tid] = ys; sZ[tid] = nz;
    // (a NaN fails both comparisons, an infinity the second)
    sUse[tid] = (fabsf(xs) <= HGS_POSE_COORD_MAX && fabsf(ys) <= HGS_POSE_COORD_MAX) ? 1 : 0;
  }
  __syncthreads();
  // ---- occlusion, confidences, the view's sum (K <= 18 values: one thread, in order)
  if (tid == 0) {
    int hidden = 0;                                  // bit k: keypoint k is hidden
    if (a.occlusion && a.occlusion[view]) {
      const int el = humansd ? 3 : 17, er = humansd ? 4 : 16, yl = humansd ? 1 : 15, yr = humansd ? 2 : 14;
      const float zn = sZ[0], zl = sZ[el], zr = sZ[er];
      if (zn > zl && zn < zr) {
        hidden |= 1 << er;
        if (sX[yr] > sX[yl]) hidden |= 1 << yr;
      } else if (zn < zl && zn > zr) {
        hidden |= 1 << el;
        if (sX[yl] < sX[yr]) hidden |= 1 << yl;
      } else if (zn > zl && zn > zr) {
        hidden |= 1 | (1 << yl) | (1 << yr);
      }
    }
    float sum = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float xs = sX[k], ys = sY[k];
      bool on = !((hidden >> k) & 1);
      if (!humansd) on = on && xs >= 0.0f && xs < (float)H && ys >= 0.0f && ys < (float)W;
      const float conf = on ? 1.0f : 0.0f;
      sConf[k] = conf;
      sum = sum + ((xs + ys) + conf);
    }
    sSumPos = sum > 0.0f ? 1 : 0;
  }
  __syncthreads();
  // ---- the records
  if (tid < R) {
    int rec[HGS_POSE_RECORD_INTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int C = 0, S = 0;
    if (humansd) {
      if (tid < a.num_limbs) {
        const int ci = a.limb[tid][0], ka = a.limb[tid][1], kb = a.limb[tid][2];
        if (sConf[ka] > 0.3f && sConf[kb] > 0.3f && sUse[ka] && sUse[kb] && sSumPos) {
          rec[0] = HGS_POSE_REC_CAPSULE;
          rec[1] = (int)sX[ka]; rec[2] = (int)sY[ka]; rec[3] = (int)sX[kb]; rec[4] = (int)sY[kb];
          rec[5] = a.limb_width;
          rec[7] = a.colour[ci][0] | (a.colour[ci][1] << 8) | (a.colour[ci][2] << 16);
        }
      }
    } else if (tid < HGS_POSE_MAX_COLOURS) {
      if (tid < K && sConf[tid] > 0.5f) {                // (masked in: inside [0, H) x [0, W), so usable)
        rec[0] = HGS_POSE_REC_DISC;
        rec[1] = (int)sX[tid]; rec[2] = (int)sY[tid]; rec[3] = 16;
        rec[7] = a.colour[tid][0] | (a.colour[tid][1] << 8) | (a.colour[tid][2] << 16);
      }
    } else if (tid - HGS_POSE_MAX_COLOURS < a.num_limbs) {
      const int i = tid - HGS_POSE_MAX_COLOURS;
      const int ci = a.limb[i][0], k0 = a.limb[i][1], k1 = a.limb[i][2];
      if (sConf[k0] > 0.5f && sConf[k1] > 0.5f) {
        const float x0 = sX[k0], x1 = sX[k1], y0 = sY[k0], y1 = sY[k1];
        const float ddx = x0 - x1, ddy = y0 - y1;
        const float length = __fsqrt_rn(ddy * ddy + ddx * ddx);
        const int theta = (int)(atan2f(ddy, ddx) * 57.29577951308232f);
        rec[0] = HGS_POSE_REC_ELLIPSE;
        rec[1] = (int)((x0 + x1) * 0.5f); rec[2] = (int)((y0 + y1) * 0.5f);
        rec[3] = (int)(length * 0.5f); rec[4] = theta; rec[5] = 4;
        rec[7] = a.colour[ci][0] | (a.colour[ci][1] << 8) | (a.colour[ci][2] << 16);
        C = HGS_POSE_COS[(theta + 720) % 360];
        S = HGS_POSE_COS[(theta + 630) % 360];
      }
    }
    if (blockIdx.x == 0) {
      int* out = a.records + ((size_t)view * R + tid) * HGS_POSE_RECORD_INTS;
#pragma unroll
      for (int i = 0; i < HGS_POSE_RECORD_INTS; ++i) out[i] = rec[i];
    }
    sRgb[tid] = rec[7];
    if (rec[0] == HGS_POSE_REC_ELLIPSE) { rec[6] = C; rec[7] = S; }
#pragma unroll
    for (int i = 0; i < HGS_POSE_RECORD_INTS; ++i) sRec[tid][i] = rec[i];
  }
  if (blockIdx.x == 0 && tid < K) {
    float* o = a.kp + ((size_t)view * K + tid) * 3;
    o[0] = sX[tid]; o[1] = sY[tid]; o[2] = sConf[tid];
  }
  __syncthreads();

  // ---- cull: the records whose box meets this tile, in order (R <= 35 < 64: the first wave, one ballot)
  const int tiles_x = (W + HGS_POSE_TILE_W - 1) / HGS_POSE_TILE_W;
  const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * HGS_POSE_TILE_W, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * HGS_POSE_TILE_H;
  if (tid < 64) {
    bool hit = false;
    if (tid < R && sRec[tid][0] != 0) {
      const int* r = sRec[tid];
      int lox, hix, loy, hiy;
      if (r[0] == HGS_POSE_REC_CAPSULE) {
        const int pad = r[5] / 2 + 1;                  // 2 d <= w
        lox = min(r[1], r[3]) - pad; hix = max(r[1], r[3]) + pad;
        loy = min(r[2], r[4]) - pad; hiy = max(r[2], r[4]) + pad;
      } else {
        // disc: radius 4.  ellipse: u^2 + v^2 <= max(a, b)^2 2^28 and C^2 + S^2 >= 2^28 - 23171, so the distance from
        // the centre is below max(a, b) (1 + 4.4e-5) < max(a, b) + 1 for a < 2^12
        const int pad = r[0] == HGS_POSE_REC_DISC ? 4 : max(r[3], r[5]) + 1;
        lox = r[1] - pad; hix = r[1] + pad; loy = r[2] - pad; hiy = r[2] + pad;
      }
      hit = hix >= tx0 && lox < tx0 + HGS_POSE_TILE_W && hiy >= ty0 && loy < ty0 + HGS_POSE_TILE_H;
    }
    const unsigned long long mask = __ballot(hit);
    if (hit) sList[__popcll(mask & ((1ull << tid) - 1ull))] = tid;
    if (tid == 0) sCount = __popcll(mask);
  }
  __syncthreads();
  const int count = sCount;

  // ---- raster: 4 consecutive pixels of a row per thread
  const int py = ty0 + tid / (HGS_POSE_TILE_W / 4), px0 = tx0 + 4 * (tid % (HGS_POSE_TILE_W / 4));
  if (py >= H || px0 >= W) return;
  int cr[4] = {0, 0, 0, 0}, cg[4] = {0, 0, 0, 0}, cb[4] = {0, 0, 0, 0};
  for (int n = 0; n < count; ++n) {
    const int s = sList[n];
    const int* r = sRec[s];
    const int rgb = sRgb[s];
    const int kr = rgb & 255, kg = (rgb >> 8) & 255, kb = (rgb >> 16) & 255;
    const bool blend = r[0] == HGS_POSE_REC_ELLIPSE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!hgs_pose_covers(r, px0 + i, py)) continue;
      if (blend) {
        cr[i] = (4 * cr[i] + 6 * kr + 5) / 10;
        cg[i] = (4 * cg[i] + 6 * kg + 5) / 10;
        cb[i] = (4 * cb[i] + 6 * kb + 5) / 10;
      } else {
        cr[i] = kr; cg[i] = kg; cb[i] = kb;
      }
    }
  }
  const int v[12] = {cr[0], cg[0], cb[0], cr[1], cg[1], cb[1], cr[2], cg[2], cb[2], cr[3], cg[3], cb[3]};
  const size_t row = ((size_t)view * H + py) * W;        // pixels in front of this row
  const size_t first = (row + px0) * 3;                  // elements in front of this thread's first
  const int npx = min(4, W - px0);
  if (a.uint8_out) {
    uint8_t* o = static_cast<uint8_t*>(a.image) + first;
    if (npx == 4 && (((uintptr_t)o) & 3) == 0) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        o4[q] = (uint32_t)v[4 * q] | ((uint32_t)v[4 * q + 1] << 8) | ((uint32_t)v[4 * q + 2] << 16) | ((uint32_t)v[4 * q + 3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * npx) o[i] = (uint8_t)v[i];
    }
  } else {
    float f[12];
    if (count == 0) {
#pragma unroll
      for (int i = 0; i < 12; ++i) f[i] = 0.0f;
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) f[i] = __fdiv_rn((float)v[i], 255.0f);
    }
    float* o = static_cast<float*>(a.image) + first;
    if (npx == 4 && (((uintptr_t)o) & 15) == 0) {
      float4* o4 = reinterpret_cast<float4*>(o);
      o4[0] = make_float4(f[0], f[1], f[2], f[3]);
      o4[1] = make_float4(f[4], f[5], f[6], f[7]);
      o4[2] = make_float4(f[8], f[9], f[10], f[11]);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * npx) o[i] = f[i];
    }
  }
}
